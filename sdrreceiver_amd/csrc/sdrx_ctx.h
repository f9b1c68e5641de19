// sdrx_ctx.h -- what a context IS: the VFO tree's nodes, the launch plans finalize leaves behind, and sdrx_ctx itself with its
// state grouped by concern; plus the error helpers every part of the host side uses.  A fragment of the one translation unit
// (sdrx.hip includes it behind the kernels); it is not a public header.
#pragma once

namespace {

thread_local std::string g_create_error;

enum Kind { KIND_MIX_ROOT = 0, KIND_MIX_SUB = 1, KIND_LATE_DEC = 2, KIND_DEMOD = 3, KIND_COMPRESS = 4, KIND_INGEST = 5, KIND_LEVELS = 6, KIND_LPF_LONG = 7 };
// The detector leaves' two block launches (detect.hip) are kinds of the leaf tail's plan only: sdrx_get_kernel_times keeps its
// SDRX_NKERNELS kinds and books them with k_compress, the payload kernel of the other non-USB leaves (bracket_kind).
constexpr int KIND_DETECT_AM = SDRX_NKERNELS, KIND_DETECT_FM = SDRX_NKERNELS + 1;
// ... and the same two for the leaves with a post-detection filter (postdet.hip): work lists of their own
constexpr int KIND_DETECT_AM_POST = SDRX_NKERNELS + 2, KIND_DETECT_FM_POST = SDRX_NKERNELS + 3;
inline int bracket_kind(int kind) { return kind >= SDRX_NKERNELS ? (int)KIND_COMPRESS : kind; }
const char *kKindNames[SDRX_NKERNELS] = {"k_mix_decimate(level0)", "k_mix_decimate(sub)", "k_late_decimate", "k_usb_demod",
                                         "k_compress",             "k_ingest",            "k_mix_levels",    "k_lpf_long"};

struct Node {
    sdrx_vfo_desc d;
    std::vector<int> children;
    int level = 0;
    int n_f = 0;       // samples of decimate[d] per frame
    int n_out = 0;     // after late decimation
    unsigned rate = 0; // outputRate
    bool leaf = false;
    // designed taps (host copies for sdrx_get_taps)
    std::vector<float> lpf, dec, hilbert;
    std::vector<float> lpf_pad, hnz; // device forms: zero-padded low-pass, compacted Hilbert
    std::vector<float> hnz_e, hnz_o; //   ... and the compacted Hilbert taps shifted by 3 / 2 in 96 zero-padded floats (hilbert4_packed)
    size_t off_hnz_e = 0, off_hnz_o = 0;
    int demod_tile = 1024;           // outputs per k_usb_demod block
    bool long_lpf = false;           // audio low-pass of more than kMaxFir taps: applied by k_lpf_long
    int Hu = 0;                      // its history length (usb floats of the previous frame)
    size_t off_u[2] = {0, 0};        // its input: [hist Hu | data n_out] usb floats per frame parity
    // device placement (byte offsets into the arena)
    size_t off_cp = 0, off_hb[2] = {0, 0}, off_stream[2] = {0, 0}, off_z[2] = {0, 0}, off_preq = 0;
    size_t off_lpf = 0, off_dec = 0, off_hilbert = 0, off_hnz = 0;
    int H = 0, Hx = 0;
    size_t pay_off = 0; // into the payload buffer
    uint32_t pay_len = 0;
    float rot_re = 0, rot_im = 0;
    int fused_late = 0;     // 5 | 6: the late decimation runs inside the mix wave (late_item); 0: not
    bool fused_demod = false; // the USB demodulation runs inside the mix wave (demod_chunk): the leaf writes its payload itself
    size_t off_dstate[2] = {0, 0}; //   ... its demodulation history per frame parity (kDemodStateFloats floats)
    int d2_index = -1;      // its K2Vfo in the demodulation descriptor array
    int d4_index = -1;      // its K4Vfo (long_lpf): k_lpf_long applies the gain
    int d2a_index = -1, d3_index = -1; // its K2aVfo (late decimation in a kernel of its own) / K3Vfo (compress): option park's flag words
    int detector = 0;       // sdrx_set_detector: kDetNone | kDetAm | kDetFm (a leaf with demod_usb = 0 only)
    int d5_index = -1;      // its K5Vfo (a detector leaf: in place of d3_index)
    size_t off_part[2] = {0, 0};  //   ... AM: the carrier's block partials per frame parity
    size_t off_zprev[2] = {0, 0}; //   ... FM: z[-1] per frame parity
    std::vector<float> post_taps; // sdrx_set_postfilter: h[0 .. T) (empty: no post-detection filter)
    int post_decim = 1;           //   ... R; the leaf leaves as n_f / R int16
    size_t off_post_taps = 0, off_post_hist[2] = {0, 0}; //   ... the taps, and pre[-(T-1) .. -1] per frame parity
    bool has_stream = true; // decimate[d] of every frame is kept in HBM (false: a fused late decimation writes only z', a fused demodulation only the payload)
    int meter_first = 0, meter_n = 0; // option meter: this leaf's records, slots [meter_first, meter_first + meter_n) behind the payloads
    int meter_shift = 0;              //   ... fuse_demod: the record of a mix item is s_first_out >> meter_shift
};

// sdrx_meter::n_values of a leaf: the int16 of a USB or a detector leaf, the two int8 a sample of an IQ leaf
inline int detect_out(const Node &n) { return n.post_taps.empty() ? n.n_f : n.n_f / n.post_decim; } // a detector leaf's int16 per frame
inline uint32_t meter_n_values(const Node &n) { return (uint32_t)(n.d.demod_usb ? n.n_out : n.detector ? detect_out(n) : 2 * n.n_f); }

struct Launch1 { // one k_mix_decimate launch (a tree level)
    int kind;
    int level;
    int n_work;
    int lds_bytes;
    size_t off_work; // arena offset of K1Work[]
    int64_t alg_bytes;
};
struct LaunchB { // block-per-tile launches (late decimate / demod / compress): one launch per kernel
    int kind;
    int n_blocks;
    size_t off_desc, off_work;
    int lds_bytes;
    int64_t alg_bytes;
    size_t off_mrel = 0; // option meter, k_lpf_long: arena offset of the blocks' record offsets (int[n_blocks])
};

// The one-launch levels (k_mix_levels): the list is [level 0 items | level 1 items | ...], every part
// starting at a multiple of 8 entries.  A launch covers the contiguous range of the levels that have a
// frame to work on.
struct LevelPlan {
    bool usable = false;
    size_t off_items = 0, off_item_level = 0, off_list = 0; // arena offsets
    std::vector<int> part_begin, part_end;                   // list range of every level
    std::vector<int64_t> part_bytes;                         // SURVEY 8d share of every level
    int lds_bytes = 0;
    // Option tail_in_levels: k_levels_tail's workgroup list [level n-1 | ... | level 0 | demodulation blocks], each part from a
    // multiple of 8 workgroups (TailWg, levels.hip); the demodulation of a frame then rides in the launch after the one that
    // finished its last level.  tail = false: k_mix_levels, and k_usb_demod behind the launch that finished the frame.
    bool tail = false;
    size_t off_wgs = 0;
    std::vector<int> wg_begin, wg_end; // workgroup range of every level
    int dm_begin = 0, dm_end = 0;      // ... and of the demodulation blocks
    int lds_wave = 0, tail_lds = 0;    // LDS of one mix wave; of a workgroup
    int64_t dm_bytes = 0;              // SURVEY 8d share of the demodulation
};
struct InFlight { // a frame inside the software pipeline: `next` = the level that runs it in the next launch (n_levels: its
                  // demodulation, with LevelPlan::tail)
    unsigned long long f;
    int next;
};

struct TimedEvent {
    hipEvent_t a, b;
    int kind;
    int64_t bytes;
};

// The buffers of a context that belong to no option (free_device_state releases them as one).
struct CtxBuffers {
    DevBuf<unsigned char> arena;
    DevBuf<unsigned char> d_pay[2]; // per frame parity
    PinBuf<unsigned char> h_pay[2];
    PinBuf<unsigned char> h_in[2];  // pinned staging of host-fed frames, per frame parity
    // host-fed frames on the device (natural order), per frame parity: frame f's buffer stays untouched until f+2 is staged
    // (another context on this device may be working on it: sdrx_submit_shared); and the same for dongle bytes.  All four or
    // none (ensure_raw).
    DevBuf<float2> d_raw[2];
    DevBuf<unsigned char> d_raw_u8[2];
    DevBuf<float2> d_raw_tiled; // the raw frame in tile layout: input of the parent-less VFOs
    DevBuf<RetuneJob> d_jobs;   // k_vfo_retune's job list (sdrx_set_mixer_freqs, sdrx_set_gains), grown on demand
};

} // namespace

struct sdrx_ctx : CtxBuffers {
    int device = 0;
    std::string err;
    std::vector<Node> nodes;
    bool finalized = false;
    int opt_exact = 1, opt_prequant = 0, opt_segments = 0, opt_dc_blocked = 0, opt_pipeline = 0, opt_dc_speculative = 1;
    int opt_fuse = 1, opt_frame_pipeline = 1, opt_fuse_late = 1, opt_keep_streams = 0, opt_fuse_demod = 0;
    int opt_tail_in_levels = 1;
    int opt_meter = 0, opt_squelch = 0, opt_preroll = 0, opt_squelch_auto = 0, opt_park = 0, opt_watch = 0, opt_catchup = 0, opt_agc = 0, opt_wake = 0;
    int opt_adc_meter = 0;
    // option meter: per frame parity, behind the payloads in d_pay / h_pay (at meter_off), one 16-byte MeterAcc record per work
    // unit that emits payload values (meter.hip "output meters"); the records travel in the payload copy
    size_t meter_off = 0;
    int meter_slots = 0;

    // Option squelch (squelch.hip): per frame parity the gate's directory sits behind the meter records in d_pay /
    // h_pay (at dir_off: SqHeader | offset per leaf | hang_left per leaf, leaves in publish order) -- [meter_off, pay_bytes) is the
    // fixed-size part that always travels -- and the open leaves' payloads are packed into d_pack[p]; the host receives them at
    // the start of h_pay[p], whose payload region they can never outgrow.
    // Option preroll: a leaf that opens in frame f after the gate closed it in f-1 is delivered with its payload
    // of f-1 in front of that of f.  prev_open per leaf on the device; the directory gains pre[n] behind hang[n]; d_pack[p] holds
    // the worst case (every leaf re-opens: twice the payload region), and so does its host side, which then lies BEHIND the
    // fixed part of h_pay[p] (at hpack_off; 0 with the option off: the start of h_pay[p], as before).
    // Option squelch_auto: the threshold follows each leaf's noise floor.  One SqAuto record per leaf on the
    // device (floor state and settings); the directory gains thr_eff[n] | floor[n] (u64) at aux_off, behind everything else.
    struct SquelchDevice { // the buffers and what describes them: what free_device_state puts back
        size_t dir_off = 0, pack_bytes = 0, hpack_off = 0;
        DevBuf<unsigned char> d_pack[2];
        DevBuf<SqLeaf> d_leaves;
        DevBuf<SqCfg> d_cfg;
        DevBuf<unsigned> d_hang; // hang_left per leaf: one array, every gate runs in frame order on one stream
        DevBuf<unsigned> d_prev; // prev_open per leaf (preroll)
        DevBuf<SqAuto> d_auto;   // floor state and settings per leaf (squelch_auto)
        DevBuf<unsigned char> d_jobs; // job list of sdrx_set_squelch (SqJob) and of sdrx_set_squelch_auto (SqAutoJob), grown on demand
        // what the option holds besides the directory (the job list is not counted)
        size_t bytes() const { return d_leaves.bytes() + d_cfg.bytes() + d_hang.bytes() + d_prev.bytes() + d_auto.bytes() + d_pack[0].bytes() + d_pack[1].bytes(); }
    };
    struct Squelch : SquelchDevice {
        int tiles = 1;                        // k_squelch_gather's grid.y: 16 KiB tiles of the longest payload
        std::vector<int> index;               // node -> its place in publish order (-1: not a leaf)
        std::vector<SqCfg> cfg;               // host copy of the thresholds
        std::vector<unsigned> offs, hang;     // the directory of the last DELIVERED frame
        unsigned n_open = 0;                  //   ... its header
        unsigned long long copied = 0;        //   ... and the payload bytes its copy moved
        unsigned long long copied_slot[2] = {0, 0};
        bool preroll_fused = false;           // a leaf demodulates in its mix wave: the levels write d_pay (enqueue_frame)
        std::vector<unsigned> pre, units;     // the delivered directory's pre-roll flags; 64-byte units of every leaf's payload
        unsigned n_pre = 0;                   // pre-rolled leaves of the delivered frame
        unsigned long long pre_bytes = 0;     //   ... and the packed bytes their pre-roll added to the copy
        size_t aux_off = 0;                   // squelch_auto: thr_eff[n] | floor[n] inside the directory (sq_aux_off)
        std::vector<SqAutoJob> acfg;          //   ... host copy of the settings (index = the leaf's place)
        std::vector<unsigned long long> thr_eff, floor; // ... the delivered directory's values (floor: kSqNone = no observation)
        hipEvent_t ev_dir[2] = {nullptr, nullptr}; // the fixed-size part of frame f is in h_pay[f & 1]
    } sq;

    // Option agc (agc.hip): one slot per USB leaf, in node order.  Per frame parity the step's records (AgcRecord per
    // slot) sit behind the meter records in d_pay / h_pay, at rec_off -- in front of the gate's directory, inside the fixed-size
    // part that always travels.  On the device the static table, the settings and quiet_run (one array: the steps run in frame
    // order on one stream, as the gates do).
    struct Agc {
        size_t rec_off = 0;
        int n = 0;                     // slots
        std::vector<int> slot;         // node -> its slot (-1: not a USB leaf)
        DevBuf<AgcLeaf> d_leaves;
        DevBuf<AgcCfg> d_cfg;
        DevBuf<unsigned> d_quiet;
        DevBuf<AgcJob> d_jobs; // job list of sdrx_set_agc, grown on demand
        size_t bytes() const { return d_leaves.bytes() + d_cfg.bytes() + d_quiet.bytes(); } // device memory the option holds besides the records and the job list
        std::vector<sdrx_agc_cfg> cfg; // host copy of the settings, per node (a compress() leaf's are stored too)
    } agc;

    // Option park (sdrx_set_active): one flag word per descriptor of every kernel that works on a leaf, in one
    // device array -- [K1Vfo: per node | K2aVfo | K2Vfo | K3Vfo | K4Vfo | K5Vfo | the gate: per leaf in publish order] -- 1 = active.
    // The host's copy of a leaf's state is what the getters and the delivery serve: a frame f >= since ran in state `active`,
    // the frames before it (the last one may not be fetched yet) in state `was_active`.  (A leaf under option wake's control is the
    // exception: the device decides, and the answers come from the frame's wake record -- leaf_parked_at, sdrx_delivery.hip.)
    struct ParkDevice { // what free_device_state releases
        DevBuf<int> d_act;
        DevBuf<unsigned char> d_jobs; // job lists of sdrx_set_active: FillJob[] | RetuneJob[], grown on demand
    };
    struct Park : ParkDevice {
        size_t o_2a = 0, o_2 = 0, o_3 = 0, o_4 = 0, o_5 = 0, o_sq = 0, words = 0;
        struct Leaf {
            int active = 1, was_active = 1;
            unsigned long long since = 0;
        };
        std::vector<Leaf> leaf; // per node (leaves only are ever changed)
        std::vector<std::vector<int>> items; // per node: its entries of LevelPlan's item_level[] (bit kParkBit; with a level plan)
        bool parked_at(int id, unsigned long long frame) const
        {
            if (leaf.empty())
                return false;
            const Leaf &L = leaf[(size_t)id];
            return !(frame >= L.since ? L.active : L.was_active);
        }
    } park;

    // Option catchup (sdrx_set_active): a leaf unparked before frame K that was parked in K-1 runs K-1 on its
    // parent's stream -- still in HBM -- before the call returns, through sub-list launches of the frame's own kernels.  Host
    // memory only: every leaf's entries of the work lists finalize built (what the sub-lists are cut from), and per leaf the
    // frame it was caught up in with that frame's meter (sdrx_get_catchup).  Empty with the option off.
    struct Catchup {
        struct Leaf {
            std::vector<K1Work> mix;        // its items of its level's k_mix_decimate launch
            std::vector<BlockWork> blk[8];  // its blocks per block kernel: 0 late decimation, 1 demodulation, 2 long low-pass, 3 compress, 4 AM detector, 5 FM detector, 6 / 7 the same with a post-detection filter
            std::vector<int> mrel;          //   ... and the record offsets of blk[2] (option meter)
            long long frame = -1;           // the frame its present active state began with a catch-up of; -1: it did not
            unsigned long long sum_sq = 0;  // that frame's meter, folded as sdrx_get_meters folds it
            uint32_t clipped = 0, peak = 0;
        };
        std::vector<Leaf> leaf; // per node
        static int slot(int kind) { return kind == KIND_LATE_DEC ? 0 : kind == KIND_DEMOD ? 1 : kind == KIND_LPF_LONG ? 2 : kind == KIND_DETECT_AM ? 4 : kind == KIND_DETECT_FM ? 5 : kind == KIND_DETECT_AM_POST ? 6 : kind == KIND_DETECT_FM_POST ? 7 : 3; }
    } cu;

    // A setting that changes between frames, as the host keeps it for what has not been delivered yet: a frame f >= since ran
    // with `v`, the frames before it (the last one may not be fetched yet) with `was`.  Only switch_to (sdrx_watch.hip) writes one.
    struct Switched {
        int v = 0, was = 0;
        unsigned long long since = 0;
        int at(unsigned long long frame) const { return frame >= since ? v : was; }
    };
    // Records of frame f: written to d[f & 1] on the device, they travel to h[f & 1] (pinned) with the frame's fixed-size part
    // (queue_watch, sdrx_delivery.hip).
    struct Records {
        DevBuf<unsigned char> d[2];
        PinBuf<unsigned char> h[2];
        size_t bytes() const { return d[0].bytes(); } // of one buffer; 0: not allocated
        hipError_t alloc(size_t n) // all four, zeroed, or none
        {
            hipError_t e = hipSuccess;
            for (int p = 0; p < 2 && e == hipSuccess; ++p)
                if ((e = d[p].alloc(n, true)) == hipSuccess)
                    e = h[p].alloc(n, true);
            if (e != hipSuccess)
                *this = Records();
            return e;
        }
        template <class R>
        R *dev(int p) const { return reinterpret_cast<R *>(d[p].get()); }
        template <class R>
        const R *host(int p) const { return reinterpret_cast<const R *>(h[p].get()); }
    };

    // Option watch (sdrx_set_watch, watch.hip).  Host bookkeeping per leaf: whether it is watched (`on`, a Switched).
    // Everything on the device is allocated by the first sdrx_set_watch that switches a leaf on; with no source measured the frame
    // sequence launches nothing more.  The records of frame f -- one slot per leaf -- are `rec`.
    // A SOURCE is what a watched leaf's band is read from: index 0 the raw frame, 1 + id the stream of node id.  Every non-leaf
    // has a slot (src_slot, in node order) for the records of the analyses below.
    struct WatchDevice { // what the first sdrx_set_watch allocates, all of it or none
        DevBuf<unsigned char> d_desc; // WatchSrc[n_src_slots] | WatchSeg[kWatchMaxSeg n_src_slots] | WatchLeaf[n_slots]
        DevBuf<unsigned char> d_data; // per measured source: P[S][kSpecN] f32 | PSD[kSpecN] + total f64 | done u32; grown on demand
        DevBuf<float2> d_tw;          // kiss_fft's twiddles, then the Hann window (as Spectrum::d_tw)
        Records rec;                  // WatchRecord[n_slots]
        size_t bytes() const { return d_desc.bytes() + d_tw.bytes() + 2 * rec.bytes() + d_data.bytes(); } // device memory the option holds
    };
    struct Watch : WatchDevice {
        struct Leaf {
            Switched on;
            int first_bin = 0, n_bins = 1; // the band (watch_band), as the descriptor stands
            int slot = -1;                 // its record (leaves in node order; -1: not a leaf)
        };
        std::vector<Leaf> leaf; // per node; sized by the first watch call (watch_host_init), as src_slot is
        int n_slots = 0;
        std::vector<int> src_slot; // per source index: its slot (-1: a leaf's stream feeds nobody)
        int n_src_slots = 0;
        std::vector<int> src_ids;        // the measured sources in launch order: -1 the raw frame, else the parent's node id
        std::vector<size_t> src_psd;     // ... where each one's PSD lies in d_data
        std::vector<int> seg_begin, leaf_begin; // per source group (0: the raw frame, 1 + l: parents on tree level l), n_levels + 2 entries
        std::vector<WatchLeaf> launch_leaves;   // the host's copy of the WatchLeaf list (what option wake's launch list is cut from)
        unsigned long long psd_since = 0; // the PSD buffers hold a frame only once frame_no > psd_since
        WatchSrc *d_src() const { return reinterpret_cast<WatchSrc *>(d_desc.get()); }
        WatchSeg *d_seg() const { return reinterpret_cast<WatchSeg *>(d_desc + sizeof(WatchSrc) * (size_t)n_src_slots); }
        WatchLeaf *d_leaf() const { return reinterpret_cast<WatchLeaf *>(d_desc + (sizeof(WatchSrc) + sizeof(WatchSeg) * kWatchMaxSeg) * (size_t)n_src_slots); }
        bool watched_at(int id, unsigned long long frame) const { return !leaf.empty() && leaf[(size_t)id].on.at(frame) != 0; }
    } watch;

    // An analysis of the watched PSD per source, part of option watch: one more kernel behind k_watch_bands on the sources that
    // have it switched on.  A source keeps what the analysis carries from frame to frame in one device allocation of its own
    // (d_state, state_bytes) from the first call that switches it on: nothing the watch moves or clears touches it.  The launch
    // list in d_desc names the sources that have it among the measured ones, rebuilt with the watch's own (walk_sources); the
    // record of frame f -- one slot per possible source, Watch::src_slot -- is in `rec`.  Everything is allocated by the first
    // call that switches a source on (analysis_alloc): sdrx_watch.hip has the shared steps.
    struct SourceAnalysis {
        struct Src {
            Switched on; // the value that switches it (0: off)
            DevBuf<unsigned char> d_state;
        };
        std::vector<Src> src; // per source index; sized by the first call
        DevBuf<unsigned char> d_desc;
        Records rec;
        size_t bytes() const // device memory it holds
        {
            size_t b = d_desc.bytes() + 2 * rec.bytes();
            for (const Src &s : src)
                b += s.d_state.bytes();
            return b;
        }
        std::vector<int> begin; // first launch entry per source group (as Watch::seg_begin), n_levels + 2 entries; empty: never switched on
    };
    // Drift estimate (sdrx_set_drift, drift.hip): switched by max_shift K.  d_state: a DriftState (template, last
    // profile, two words of launch state); d_desc: DriftSrc[n_src_slots] | DriftBlk[kDriftMaxBlocks n_src_slots]; rec: DriftRecord.
    struct Drift : SourceAnalysis {
        std::vector<unsigned long long> set_at; // per source index: frame_no of the last sdrx_set_drift -- the profile is this setting's once frame_no > set_at
        DriftSrc *d_src() const { return reinterpret_cast<DriftSrc *>(d_desc.get()); }
        DriftBlk *d_blk(int n_src_slots) const { return reinterpret_cast<DriftBlk *>(d_desc + sizeof(DriftSrc) * (size_t)n_src_slots); }
    } drift;
    // Band scan (sdrx_set_scan, scan.hip): switched by the cell width cell_bins.  d_state: a ScanState (integrated
    // spectrum, count, and the cells, hits and record of the last completed evaluation); d_desc: ScanSrc[n_src_slots]; rec: ScanRecord.
    struct Scan : SourceAnalysis {
        std::vector<ScanCfg> cfg; // per source index: the setting that last switched it on
        ScanSrc *d_src() const { return reinterpret_cast<ScanSrc *>(d_desc.get()); }
    } scan;

    // Option wake (sdrx_set_wake, wake.hip): the leaves the device parks and unparks itself.  `ctl` says per leaf
    // whether it is under control (a Switched); for a frame it is, whether the leaf ran is a device result -- the wake record of
    // that frame (`rec`, one slot per leaf: the watch's slots), not Park::leaf (leaf_parked_at, sdrx_delivery.hip).  Everything on
    // the device is allocated by the first sdrx_set_wake that switches a leaf on: the static table and the state per watch slot,
    // the launch list (the controlled leaves in the order of the watch's own list, `begin` per source group as
    // Watch::leaf_begin) and the fill lists of the controlled leaves (leaf_regions, sdrx_wake.hip).
    struct WakeDevice { // what the first sdrx_set_wake that switches a leaf on allocates, all of it or none
        DevBuf<WakeLeaf> d_leaf;
        DevBuf<WakeState> d_state;
        DevBuf<int> d_list;
        DevBuf<WakeFill> d_fill; // grown on demand
        Records rec;             // WakeRecord per watch slot
        size_t bytes() const { return d_state.bytes() + d_list.bytes() + d_leaf.bytes() + 2 * rec.bytes() + d_fill.bytes(); } // device memory the option holds
    };
    struct Wake : WakeDevice {
        std::vector<Switched> ctl;      // per node; sized by the first sdrx_set_wake
        std::vector<sdrx_wake_cfg> cfg; // per node: the settings as set
        int n_ctl = 0;                  // leaves under control
        std::vector<WakeLeaf> h_leaf;   // host copy of d_leaf
        std::vector<int> begin;         // first launch entry per source group, n_levels + 2 entries
        bool controlled(int id) const { return !ctl.empty() && ctl[(size_t)id].v != 0; }
        bool controlled_at(int id, unsigned long long frame) const { return !ctl.empty() && ctl[(size_t)id].at(frame) != 0; }
    } wake;

    // Option adc_meter (adcmeter.hip): exact integer statistics of every frame that reaches the context as integer
    // samples.  Allocated at sdrx_finalize with the option on: one AdcPartial per workgroup of the longest frame, the launch's
    // counter, and the record of frame f (`rec`, one AdcRecord).  A frame that is not measured launches nothing, so its slot
    // holds stale bytes: `note` says per frame parity which frame the slot was last written for and in which format, and the
    // getter answers from it.
    struct AdcDevice { // what free_device_state releases
        DevBuf<AdcPartial> d_part;
        DevBuf<unsigned> d_count;
        Records rec;
        size_t bytes() const { return d_part.bytes() + d_count.bytes() + 2 * rec.bytes(); } // device memory the option holds
    };
    struct Adc : AdcDevice {
        struct Note {
            unsigned long long frame = 0;
            int fmt = -1; // -1: nothing measured yet
        } note[2];
    } adc;

    // An ingest stage with settings and a record of every frame (blanker, IQ balance, shift, spur canceller): `Device` is what
    // finalize allocates with it and free_device_state releases, its `rec` the record of frame f.  `used` says per frame parity
    // which frame the slot was written for and under which settings: what the stage's getter answers from.
    template <class Cfg, class Device>
    struct CfgStage : Device {
        bool on = false; // set before sdrx_finalize
        Cfg cfg{};       // the settings of the next frame
        struct Used {
            unsigned long long frame = 0;
            bool any = false;
            Cfg cfg{};
        } used[2];
        void ran(int p, unsigned long long frame) { used[p] = Used{frame, true, cfg}; } // the stage's launch: frame `frame` passed it
        void reset_used() { used[0] = used[1] = Used(); }
    };

    // Resampler (sdrx_set_resampler, resample.hip): frames arrive at the rate fs_in, in_frame samples each, and
    // k_resample makes the tree's raw frame (root_frame samples in d_raw_tiled) from them.  The setting -- the rate and the
    // caller's taps in prototype order, or why that ratio is not offered -- is the host's and stays; what finalize allocates
    // with it: the input-rate frame in tile layout (where the ingest kernels then write), the history of both frame parities
    // (kRsHist cf32 each, zeroed), and the taps phase-major.
    struct ResamplerDevice { // what free_device_state releases
        DevBuf<float2> d_stage;
        DevBuf<float2> d_hist;
        DevBuf<float> d_taps;
        size_t bytes() const { return d_stage.bytes() + d_hist.bytes() + d_taps.bytes(); } // device memory it holds
    };
    struct Resampler : ResamplerDevice {
        bool on = false;          // set (sdrx_set_resampler with fs_in > 0)
        ResamplePlan plan;        // the ratio from the setting, the frame lengths from finalize
        std::string refused;      // not empty: why finalize will refuse the ratio (no taps were copied)
        std::vector<float> taps;  // L T floats, prototype order
        double passband_hz = 0;
        int lds_bytes = 0;        // k_resample's dynamic LDS: the output tile and the longest window
    } rs;
    // Front stage (sdrx_set_front, front.hip): 1 .. 3 half-band decimations by 2 in front of the resampler, or of
    // level 0 where none is set; stage 1 may read real samples.  The setting is the host's and stays; what finalize allocates
    // with it: the cf32 input frame of every complex stage in tile layout (d_in[s - 1] for stage s; stage 1 of a real front end
    // reads the caller's words and has none), every stage's history of both frame parities (kFrHist cf32 each, zeroed) and the
    // non-zero taps.  The last stage writes the resampler's staging buffer or the tree's raw frame.
    struct FrontDevice { // what free_device_state releases
        DevBuf<float2> d_in[kFrMaxStages];
        DevBuf<float2> d_hist;
        DevBuf<float> d_taps;
        size_t bytes() const { return d_in[0].bytes() + d_in[1].bytes() + d_in[2].bytes() + d_hist.bytes() + d_taps.bytes(); }
    };
    struct Front : FrontDevice {
        bool on = false;         // set (sdrx_set_front)
        FrontPlan plan;          // the setting, the frame lengths from finalize
        std::vector<float> taps; // N floats, prototype order
        double tw = 0;           // the built-in design's transition width (0 for the caller's own taps)
    } fr;
    // Impulse blanker (sdrx_set_blanker, blank.hip): k_blank between the ingest kernels and what they wrote before.
    // The setting is the host's; what finalize allocates with it: the staging frame the ingest kernels then write (tile layout),
    // the device state (reference bin, carry, the frame's histogram and counters) and the record of frame f (`rec`).
    struct BlankerDevice { // what free_device_state releases
        DevBuf<float2> d_stage;
        DevBuf<BlankState> d_state;
        Records rec;
        size_t bytes() const { return d_stage.bytes() + d_state.bytes() + 2 * rec.bytes(); } // device memory it holds
    };
    CfgStage<BlankCfg, BlankerDevice> bl;
    bool staged() const { return rs.on || fr.on || bl.on; } // the ingest kernels write a staging buffer, not the tree's raw frame
    // IQ balance correction (sdrx_set_iq_balance, iqbal.hip): k_iqbal in place on what the ingest kernels wrote, in
    // front of the blanker.  The setting is the host's; what finalize allocates with it: the device state (the pair and the five
    // accumulators of the frame in flight) and the record of frame f (`rec`).  No staging frame: staged() is not its business,
    // but every frame, cf32 ones included, then takes the ingest pass into the tile layout (tiled_ingest).  cfg.c0, cfg.d0: what
    // sdrx_finalize or the last SDRX_IQ_LOAD wrote.
    struct IqDevice { // what free_device_state releases
        DevBuf<IqState> d_state;
        Records rec;
        size_t bytes() const { return d_state.bytes() + 2 * rec.bytes(); } // device memory it holds
    };
    CfgStage<IqCfg, IqDevice> iq;
    // Frequency shift (sdrx_set_shift, shift.hip): k_shift in place on the tree's raw frame, behind the resampler or
    // whatever comes last in the ingest chain.  The setting is the host's; what finalize allocates with it: the device state (phase
    // and increment of the next frame), the one device copy of the three tables and the record of frame f (`rec`).  No staging
    // frame, but every frame takes the ingest pass into the tile layout (tiled_ingest).  cfg.inc: of the next frame; cfg.phase0:
    // what sdrx_finalize or the last SDRX_SHIFT_LOAD_PHASE wrote.
    struct ShiftDevice { // what free_device_state releases
        DevBuf<ShiftState> d_state;
        DevBuf<float2> d_tab; // A | B | C, 3 * kShTab entries
        Records rec;
        size_t bytes() const { return d_state.bytes() + d_tab.bytes() + 2 * rec.bytes(); } // device memory it holds
    };
    CfgStage<ShiftCfg, ShiftDevice> sh;
    // Spur canceller (sdrx_set_notch, notch.hip): k_notch_corr / _step / _apply in place on the tree's raw frame, in
    // front of k_shift.  What finalize allocates with it: the eight tone slots, c[b][k] and used[b][k] of one frame's blocks, the
    // record of frame f (`rec`) and -- unless the shift is on, whose copy then serves both (shift_tables_dev) -- the three tables.
    // cfg: as last written (flags: of the last call), and what the getter answers with -- used[].cfg goes unread.
    struct NotchDevice { // what free_device_state releases
        DevBuf<NotchTone> d_state;  // kNtMax slots
        DevBuf<ShiftC> d_c, d_used; // blocks * kNtMax each
        DevBuf<float2> d_tab;       // A | B | C; empty with the shift on
        Records rec;
        size_t bytes() const { return d_state.bytes() + d_c.bytes() + d_used.bytes() + d_tab.bytes() + 2 * rec.bytes(); }
    };
    CfgStage<NotchCfg, NotchDevice> nt;
    const float2 *shift_tables_dev() const { return sh.on ? sh.d_tab.get() : nt.d_tab.get(); } // the one device copy of A | B | C
    bool tiled_ingest() const { return staged() || iq.on || sh.on || nt.on; } // every frame goes through an ingest kernel into the tile layout
    int in_frame = 0; // samples of an incoming frame: root_frame, or with a resampler rs.plan.n_in; times 2^stages with a front stage
    // Where the out-of-place kernels of the ingest chain write, in tile layout: planned once by sdrx_finalize (plan_ingest_route,
    // sdrx_finalize.hip, which states the whole routing), cleared by free_device_state with the buffers it points into.
    struct IngestRoute {
        float2 *ingest_out = nullptr; // the format conversion (and the DC forms); the IQ balance works in place on it
        float2 *blank_out = nullptr;  // k_blank, reading its staging frame
        float2 *front_out = nullptr;  // the last front stage
    } route;

    // sdrx_set_tap / sdrx_add_tap: the fused late-decimation leaves that keep decimate[0] because they are taps (vfo::fftVFOSlot
    // sets emitFFT on EVERY VFO whose topic matches, vfo.cpp:492-509): node -> its buffers per frame parity and the first
    // frame that fills them.  The first such leaf uses the arena's buffer, further ones buffers of their own (`own`).
    struct TapBuf {
        float2 *buf[2] = {nullptr, nullptr};
        unsigned long long since = 0;
        DevBuf<float2> own[2]; // what buf[] points at, unless it is the arena's
    };
    std::map<int, TapBuf> taps;
    size_t tap_len = 0, off_tapbuf[2] = {0, 0}; // the arena's tap buffer (sized for the longest fused leaf), per frame parity
    LevelPlan fp;
    std::vector<InFlight> pipe; // oldest first
    sdrx_publish_fn cb = nullptr;
    void *cb_user = nullptr;

    // Streams.  `stream` (the context's own or the caller's) carries the ingest and the
    // mix/decimate launches of every tree level; the leaf tail of a frame runs on `tail_stream`
    // when option "pipeline" is on (off by default: measured slower, profiles/README.md); payloads leave on
    // `copy_stream` for frames that came in through sdrx_submit*.  Cross-stream order is by the
    // per-parity events below (measured on this runtime, tools/event_probe.hip: a record costs its
    // stream ~3-5 us, a wait on an event that completed long ago ~2.5 us, a tight hop ~11 us).
    struct Streams {
        hipStream_t own_stream = nullptr, stream = nullptr, tail_stream = nullptr, copy_stream = nullptr, copy_stream2 = nullptr; // copy_stream2: odd frames
        hipEvent_t ev_levels[2] = {nullptr, nullptr}; // levels of frame f done (recorded on `stream`)
        hipEvent_t ev_tail[2] = {nullptr, nullptr};   // tail of frame f done (recorded on the tail's stream)
        hipEvent_t ev_copied[2] = {nullptr, nullptr}; // payloads of frame f are in h_pay[f & 1]
        hipEvent_t ev_staged[2] = {nullptr, nullptr}; // the host frame of parity p is complete on the device
        bool tail_recorded[2] = {false, false};
    } st;
    bool long_frame = false;             // the frame's kernels outlast its payload copy (the DC-bias recurrence): the copy is issued by sdrx_wait
    bool copy_owed[2] = {false, false};  //   ... and not issued yet
    size_t arena_bytes = 0;
    size_t pay_bytes = 0;
    int in_flight = 0;               // frames submitted (sdrx_submit*) and not yet delivered (sdrx_wait)
    bool broken = false;             // fault injection (SDRX_FAULT_WAIT): every frame call fails from here on, like after a HIP error
    int host_slot = -1;              // which h_pay holds the payloads sdrx_get_output serves
    unsigned long long host_frame = 0; // ... and which frame they are
    // other contexts that ran on this context's uploaded frame of parity p (sdrx_submit_shared): each left an event behind its
    // kernels, and this context's next upload into that buffer waits for them (events owned, and reused, by this context).
    // No lock: `ctx` and `src` of a sharing call must be driven from ONE thread (sdrx.h).
    struct SharedReader {
        const sdrx_ctx *who; // (identity only: never dereferenced)
        hipEvent_t ev;       // behind who's kernels on this context's frame of that parity; owned by THIS context
        bool pending;        // recorded since this context last waited for it
    };
    std::vector<SharedReader> shared_readers[2]; // at most one entry per (reader, parity): re-recorded, never piled up
    int last_raw = -1;             // how the last frame reached level 0 (kRaw*; -1: caller-owned device memory)
    bool late4 = false;            // k_late_decimate4 serves the late-decimation launch
    bool root_direct = false;      // level 0 reads the caller's natural-order frame itself (few VFOs)
    struct DcDevice { // DC-bias removal of dongle bytes (sdrx_*_u8 with correct_dc), allocated by the first such frame (dc_first_use)
        DevBuf<float> d_state;      // accumulator (exact: [2]; fast: [parity][2])
        DevBuf<float> d_work;       // exact removal: products P[2][stride] and estimates A[2][stride] of one frame
        DevBuf<unsigned long long> d_counters; // k_dc_chain_spec: [0] blocks walked, [1] blocks redone with the sequential operations, [2] blocks taken again on their own
        int work_stride = 0;
        DevBuf<double> d_tab;       // fast scan: powers of the decay + per-chunk sums behind them
        unsigned long long frames = 0; // frames the fast scan has run on (its state ping-pongs)
        size_t tab_sums = 0;        // offset (in doubles) of the double2 sums[] inside d_tab
    };
    struct DcBias : DcDevice {
        int waves = 8;              // k_dc_chain_spec: blocks per step = waves per workgroup (option dc_blocks_per_step: 1, 2, 4, 8)
    } dc;
    int root_frame = 0; // samples_per_buffer of the parent-less VFOs
    size_t off_k1vfo = 0;
    size_t off_k2 = 0, off_k4 = 0, off_k5 = 0; // the K2Vfo / K4Vfo / K5Vfo arrays (sdrx_set_gains patches their gain)
    size_t off_k5post = 0;                     // the K5Post array beside K5Vfo's (only with a post-detection filter somewhere)
    std::vector<Launch1> l1;
    std::vector<LaunchB> lb;
    std::vector<int> publish_order;
    unsigned long long frame_no = 0;
    bool pending_fetch = false;
    int64_t alg_bytes = 0, vfo_samples = 0, mix_chunks = 0;
    int n_levels = 0;

    struct Timing { // sdrx_enable_kernel_timing: an event pair around every launch (Bracket, sdrx_frame.hip)
        bool on = false;
        std::vector<TimedEvent> pending;
        std::vector<hipEvent_t> pool;
        double ms[SDRX_NKERNELS] = {0};
        int64_t n[SDRX_NKERNELS] = {0};
        int64_t bytes[SDRX_NKERNELS] = {0};
    } tm;

    // spectrum display (sdrx_set_spectrum): state slot id of a VFO, nodes.size() of the raw frame.  All of it is allocated by
    // sdrx_set_spectrum; with nothing enabled the frame sequence launches nothing more.
    struct SpecState {
        DevBuf<double> pwr; // kSpecN doubles, then kSpecN cf32 bins (one allocation, counted in doubles)
        bool on = false;
    };
    struct Spectrum {
        std::vector<SpecState> slots;  // per slot
        DevBuf<SpecRecord> d_rec;      // per slot (one array: sdrx_get_spectrum_levels is one copy)
        DevBuf<float2> d_tw;           // kiss_fft's twiddles, then the Hann window (kSpecN floats)
        DevBuf<SpecDesc> d_desc;       // the VFO spectra that have a stream, by tree level; then the raw one
        int n_desc = 0;                // VFO descriptors in d_desc
        std::vector<int> level_begin;  // first descriptor of every level (n_levels + 1 entries)
        bool raw_on = false;
        int raw_count = 0;             // sdrj's `count` (sdrj.cpp:84-101, 296-303)
    } spec;
};

namespace {

int fail(sdrx_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c)
        c->err = buf;
    else
        g_create_error = buf;
    return code;
}

#define HIPCHK(c, expr)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail((c), SDRX_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct ArenaPlan {
    size_t size = 0;
    size_t take(size_t bytes)
    {
        size_t o = align_up(size, 256);
        size = o + bytes;
        return o;
    }
};

} // namespace
