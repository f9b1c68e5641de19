// sdrx_dev.h -- device-visible descriptors shared by the kernels and the host orchestration.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdrx {

constexpr int kRun = 16;            // input samples per lane per chunk (NCO checkpoint spacing)
constexpr int kChunk = 64 * kRun;   // 1024 input samples per wave-iteration
constexpr int kCarry = 16;          // per-stage history window kept in LDS between chunks
constexpr int kHbHist = 10;         // half-band history carried between frames (x[-1..-10])
constexpr int kMaxStages = 8;       // vfo.h:63
constexpr int kMaxLevels = 4;       // tree depth up to which k_mix_levels (all levels in one launch) is used (the reference builds 2)
constexpr int kHilbert = 125;       // vfo.cpp:137
constexpr int kHilbertNz = 62;      // non-zero Hilbert taps (odd indices 1..123)
constexpr int kDelay = 62;          // vfo.cpp:136
constexpr int kMaxFir = 256;        // longest low-pass k_usb_demod applies itself (staged in LDS); longer ones: k_lpf_long
constexpr int kMaxFirLong = 8192;   // longest low-pass at all (window + block in LDS: 33 KB)
// where the parent-less VFOs of a launch read the raw frame from
constexpr int kRawTiled = 0;        // the context's tile-layout copy (an ingest kernel wrote it)
constexpr int kRawF32 = 1;          // the caller's cf32 frame, natural order
constexpr int kRawU8 = 2;           // the dongle's interleaved bytes, natural order

// TILE LAYOUT.  Every cf32 stream that feeds k_mix_decimate is stored in tiles of 1024 samples:
// tile c is 512 float4 units [i2 = 0..7][lane = 0..63]; unit (i2, lane) holds samples
// c*1024 + lane*16 + 2*i2 and +1.  A wave then loads its chunk as 8 fully coalesced 1 KiB
// instructions and every lane ends up with 16 CONSECUTIVE samples in registers -- the shape both
// the NCO replay and the register-resident half-band stages want -- with no LDS transpose.
__device__ __forceinline__ size_t tile_unit(int chunk, int i2, int lane) { return (size_t)chunk * 512 + i2 * 64 + lane; }
// float2 index of natural sample g inside a tile-layout stream; T: the index type the caller computes in (the kernels of
// mix.hip address with size_t, k_spectrum's and the watch's sample fetch with int)
template <typename T>
__host__ __device__ constexpr T tile_index(int g)
{
    const int c = g >> 10, r = g & 1023, ln = r >> 4, i = r & 15;
    return (T)c * 1024 + (i >> 1) * 128 + ln * 2 + (i & 1);
}
// host: the first n samples of a tile-layout stream (whole tiles, copied from the device) in natural order, as the getters of
// include/sdrx.h hand them out: interleaved floats, no alignment asked of `out` beyond a float's
inline void untile(const float2 *tiled, float *out, int n)
{
    for (int g = 0; g < n; ++g) {
        const float2 v = tiled[tile_index<size_t>(g)];
        out[2 * g] = v.x;
        out[2 * g + 1] = v.y;
    }
}

struct K2Vfo;
// ---- mix + half-band cascade (one per VFO) ---------------------------------------------------
struct K1Vfo {
    const float2 *in[2];   // input stream in TILE LAYOUT (above) per frame parity
    float2 *out[2];        // decimate[d] of this frame, per frame parity (tile layout iff out_tiled)
    const float2 *cp;      // NCO checkpoints: cp[j] = table[16 j - 1], cp[0] = (1,0), cp[L/16] = table[L-1]
    float2 *hb[2];         // half-band history per frame parity: [d][10], entry k-1 = x[-k]
    float rot_re, rot_im;  // NCO rotation (float cos, float sin of the double angle)
    int n_in;              // complex samples per frame
    int d;                 // half-band stages
    int L;                 // NCO table length = (int)fs
    int out_tiled;         // 1: children consume the output (tile layout); 0: natural order for the demod
    // A leaf whose /5 or /6 low-pass (vfo::usb_decimdemod, vfo.cpp:334-387) runs in the mix wave itself (late_item, mix.hip):
    // d == 0, `out` = the DECIMATED stream z' (behind its demodulation history), hb[] = the last kLateHist mixed samples of
    // the previous frame, and the mixed 240 kS/s stream decimate[0] is never written to HBM -- unless it is wanted:
    int late_L;            // 0: not such a leaf; 5 | 6
    int pad_;
    const float *late_taps; // the Nd = LateGeom<L>::kTaps taps of the decimating low-pass
    float2 *tap[2];        // non-null: also keep decimate[0] of this frame here, natural order (sdrx_set_tap, option keep_streams)
    // Tolerance arithmetic only (option exact = 0; nco.hip "NCO in the tolerance arithmetic"): rk[j] = u^(j+1), u = the
    // rotation by the angle of (rot_re, rot_im) at unit modulus, computed in double and stored as floats -- 1 .. 4 steps of
    // the table's recurrence as one rotation, once its amplitude has settled (entries >= kNcoSettle).
    float2 rk[4];
    // A USB leaf that demodulates in the mix wave itself (demod_chunk, demod.hip; option fuse_demod): its demodulation
    // descriptor.  `out` is then unused -- decimate[d] of such a leaf goes to HBM only through `tap`.
    const K2Vfo *dm;
    // The frame at which this VFO's oscillator started: 0 at finalize, the next frame after sdrx_set_mixer_freqs.  The table
    // phase of frame f is ((f - origin) n_in) mod L, and sample 0 of frame `origin` takes the table's last entry -- a fresh
    // Oscillator (oscillator.cpp:20-50) from that frame on.  (A frame number: as wide as the one the kernels are given.)
    unsigned long long origin;
};
static_assert(sizeof(K1Vfo) % 8 == 0, "K1Vfo array stride");
constexpr int kNcoSettle = 512; // table entries below this still carry the start-up ringing of the amplitude stabiliser (oscillator.cpp:20-28): always replayed exactly

// Geometry of the fused late decimation for L in {5, 6}.  The decimating low-pass is low_pass(2, rate L, rate / 2, rate / (L - 1))
// (vfo.cpp:82-87): its length (int)(53 fs / (22 tw)) made odd depends on fs / tw = L (L - 1) only -- 49 taps for L = 5, 73 for
// L = 6, whatever the rate (checked at finalize; anything else takes the two-kernel path).  A wave walks its segment in chunks
// of kChunkLen samples (a multiple of 16 L, so that a chunk starts on an output and a lane's 16-sample run on a run of the
// tile layout) = kMixLanes lanes of 16 consecutive samples for the NCO and the mixer, and = kRows rows of 3 L samples for the
// FIR: lane l then owns the three outputs whose newest-but-one sample lies in row l.
template <int L>
struct LateGeom;
template <>
struct LateGeom<5> {
    static constexpr int kTaps = 49, kRow = 15, kRows = 64, kChunkLen = 960, kMixLanes = 60;
    static constexpr int kStride = 18;    // LDS row stride in samples: 9 slots of 16 bytes -> the 16 lanes of a ds_read_b128 group hit 16 distinct slots,
                                          //   and the 16 lanes of a ds_write_b64 group (pad 3: 6 dwords per row crossed) 16 distinct bank pairs
                                          //   (17 -- 9.3 KB of LDS per wave, 17 instead of 16 waves per CU, single b64 window reads --
                                          //   measured slower: 0.0512 vs 0.0505 ms exact, 0.0419 vs 0.0392 tolerance; profiles/README.md round 6)
    static constexpr int kCarryRows = 4;  // rows of the previous chunk a window reaches back into: 4 x 15 >= 49
    static constexpr int kWarm = 80;      // a segment that starts inside the frame walks this many samples first: >= kTaps, a multiple of 16 L
};
template <>
struct LateGeom<6> {
    static constexpr int kTaps = 73, kRow = 18, kRows = 56, kChunkLen = 1008, kMixLanes = 63;
    static constexpr int kStride = 19;    // 38 dwords
    static constexpr int kCarryRows = 5;  // 5 x 18 >= 73
    static constexpr int kWarm = 96;
};
template <int L>
__host__ __device__ constexpr int late_hist() { return LateGeom<L>::kCarryRows * LateGeom<L>::kRow; } // samples carried between frames
constexpr int kLateTapPad = 80; // the taps in LDS, zero-padded to whole float4s
template <int L>
__host__ __device__ constexpr int late_window_bytes() // [carry rows | chunk rows], rounded up to 16 bytes
{
    return (8 * (LateGeom<L>::kCarryRows + LateGeom<L>::kRows) * LateGeom<L>::kStride + 15) / 16 * 16;
}
template <int L>
__host__ __device__ constexpr int late_lds_bytes() { return late_window_bytes<L>() + 4 * kLateTapPad; }

// One wave's job: samples [s_begin, s_end) of one VFO-frame, walked in 1024-sample chunks (all three
// are multiples of 16 and of 2^d; s_end - s_begin is a whole number of chunks except at the frame's
// end).  A segment that starts inside the frame starts from zero filter state: its outputs are exact
// from input position s_first_out = s_begin + warm-up on, and only those are emitted.
struct K1Work {
    int vfo;
    int s_begin, s_first_out, s_end;
};

// One block's job in the block-per-tile kernels (late decimation, demod, compress).
struct BlockWork {
    int vfo; // index into that kernel's descriptor array
    int blk; // tile index within the VFO-frame
};

// ---- late decimation by L (vfo::usb_decimdemod, vfo.cpp:334-387) ------------------------------
struct K2aVfo {
    const float2 *x[2];     // [hist Hx | data n] per parity
    float2 *x_next[2];      // the other parity's buffer (history for the next frame)
    float2 *z[2];           // output stream data base (after ITS history) per parity
    const float *taps;      // Nd taps
    int Hx, n, ndec, L;
    int n_out;              // n / L
    int pad_;
};

// ---- USB demod + audio low-pass + int16 (vfo::usb_demod, vfo.cpp:300-332) ---------------------
struct K2Vfo {
    const float2 *s[2];     // [hist H | data n] per parity
    float2 *s_next[2];
    const float *hnz;       // the 62 non-zero Hilbert taps hp[1], hp[3], ..., hp[123]
    const float *lpf_pad;   // audio low-pass taps with 3 zeros in front and >= 8 behind, or null
    short *pay[2];          // n int16, per frame parity (frame f's payload is copied out while f+1 is computed)
    float *prequant;        // optional n floats
    float gain;
    int H, n, nlpf;
    int tile;               // outputs per block: 1024, or 1024 - E with the low-pass (E = nlpf rounded up to even)
    int meter_rel;          // option meter: byte offset from pay[par] to this leaf's first output-meter record (a multiple of 16); a
                            //   leaf that demodulates in its mix wave keeps s in the low 4 bits: its item from input sample
                            //   s_first_out writes record s_first_out >> s
    float *usb_out[2];      // a low-pass longer than kMaxFir: the unfiltered usb floats go here per frame parity
                            //   (behind that stream's history) and k_lpf_long does the rest; else null
    const float *hnz_e, *hnz_o; // the same taps for the packed MACs of the non-exact arithmetics (hilbert4_packed): hnz_e[m] = h[m-3],
                            //   hnz_o[m] = h[m-2] with h[s] = hnz[s], zeros outside 0 .. 61; 96 floats each
    float *state[2];        // a leaf that demodulates in its mix wave: its demodulation history per frame parity (256 floats:
                            //   the last 62 odd / 62 even Q, 62 I and Nh usb values at 64-float strides); else null
};
static_assert(sizeof(K2Vfo) % 8 == 0, "K2Vfo array stride");

// ---- compress() for childless non-USB VFOs (vfo.cpp:389-424) ----------------------------------
struct K3Vfo {
    const float2 *s[2];
    signed char *pay[2];    // per frame parity
    int n, cstyle, scalecomp;
    int meter_rel;          // option meter: byte offset from pay[par] to this leaf's first output-meter record (one per block)
};

// ---- audio low-pass of more than kMaxFir taps (FIR::FIRUpdateAndProcess, dsp.cpp:59-71) + int16 --------
struct K4Vfo {
    const float *u[2];      // [hist Hu | data n] usb floats per frame parity
    float *u_next[2];       // the other parity's buffer (history for the next frame)
    const float *taps;      // nlpf taps
    short *pay[2];
    float *prequant;
    float gain;
    int Hu, n, nlpf;
};

// ---- detector leaves: AM envelope / FM discriminator of a childless non-USB VFO's stream (detect.hip, sdrx_detect.h) ----------
struct K5Vfo {
    const float2 *s[2];          // the leaf's stream per frame parity (no history in front: 16-byte aligned)
    short *pay[2];               // n int16, per frame parity
    unsigned long long *part[2]; // AM: one partial of the carrier sum per block and frame parity (k_env_sum writes, k_detect<AM> adds)
    float2 *zprev[2];            // FM: z[-1] of the frame of this parity (the tail of the frame before wrote it; zero for a new vfo)
    float gain;
    int n;                       // stream samples per frame
    int kind;                    // kDetAm | kDetFm (sdrx_detect.h)
    int meter_rel;               // option meter: byte offset from pay[par] to this leaf's first output-meter record (one per block)
};
static_assert(sizeof(K5Vfo) % 8 == 0, "K5Vfo array stride");

// ---- the post-detection filter of a detector leaf (postdet.hip, sdrx_postdet.h): an array beside K5Vfo's, entry for entry, that
// exists only where some leaf has the filter (K5Vfo and what a tree without one allocates stay what they were)
struct K5Post {
    const float *taps; // h[0 .. ntaps)
    float *hist[2];    // pre[-(ntaps-1) .. -1] of the frame of this parity (the tail of the frame before wrote it; zero for a new vfo)
    int ntaps, decim;  // 0, 0: this leaf has no filter (it is on k_detect's lists)
};
static_assert(sizeof(K5Post) % 8 == 0, "K5Post array stride");

struct NcoInit {
    float2 *cp;
    float rot_re, rot_im;
    int L;
    int pad_;
};

// One entry of k_vfo_retune's job list (sdrx_set_mixer_freqs, sdrx_set_gains).
constexpr int kJobRetune = 0; // a new oscillator: regenerate vfo->cp, then write rot, rk and origin into *vfo
constexpr int kJobGain = 1;   // *gain = value (K2Vfo::gain, K4Vfo::gain or K5Vfo::gain)
struct RetuneJob {
    K1Vfo *vfo;
    float *gain;
    float rot_re, rot_im;
    float2 rk[4];
    unsigned long long origin;
    int kind;
    float value;
};
static_assert(sizeof(RetuneJob) % 8 == 0, "RetuneJob array stride");

// ---- option park (sdrx_set_active) ----------------------------------------------
// What the park = 1 form of a kernel is given besides, in a trailing argument that is empty for the form without: the option
// off runs the kernels as they were.  `act`: one word per descriptor of THAT kernel (K1Vfo: per node; K2aVfo / K2Vfo / K3Vfo /
// K4Vfo / K5Vfo: per entry of the array; the squelch gate: per leaf in publish order), 1 = active, 0 = parked.  A work unit reads its
// word first -- wave-uniform, a scalar load -- and returns if it is 0.
// The mix items of the one-launch levels (k_mix_levels, k_levels_tail) carry the flag in a word they read anyway: bit kParkBit
// of their entry of item_level[] is set while the leaf is parked (the exact k_levels_tail has no register for another pointer;
// its `act` names the K2Vfo words of its demodulation blocks).
constexpr int kParkBit = 1 << 8;
template <bool PARK>
struct ParkArg {
};
template <>
struct ParkArg<true> {
    const int *act;
};

// One entry of k_vfo_reset's job list: `words` 32-bit words from `ptr` on become `value` -- a flag word (1 word), a state
// region of a leaf that is unparked (zeros: the reference's zero-initialised filter state, dsp.cpp:40-49), its gate state.
struct FillJob {
    unsigned *ptr;
    unsigned words, value;
};
static_assert(sizeof(FillJob) == 16, "FillJob array stride");

} // namespace sdrx
