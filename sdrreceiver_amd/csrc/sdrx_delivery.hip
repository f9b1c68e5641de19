// sdrx_delivery.hip -- how a frame's payloads reach the host and the caller: the egress copies, sdrx_wait / sdrx_fetch, the
// publish callbacks, and the calls that read the delivered frame (output, meters, squelch, egress, pre-roll).
// A fragment of sdrx.hip's translation unit.

namespace {

// Option wake: the wake record of leaf `id` for frame `frame`, if the leaf was under the device's control in that frame -- from
// the pinned copy that travelled with the delivered frame, else one small device read (the caller has seen that frame's
// kernels end: a delivered frame, or a drained context).  false: not controlled then, or the record is no longer that frame's.
bool wake_record(const sdrx_ctx *c, int id, unsigned long long frame, WakeRecord *out)
{
    const sdrx_ctx::Wake &K = c->wake;
    if (!K.controlled_at(id, frame) || !K.rec.d[0])
        return false;
    const int slot = c->watch.leaf[(size_t)id].slot, p = (int)(frame & 1ull);
    if (c->host_slot == p && c->host_frame == frame) {
        *out = K.rec.host<WakeRecord>(p)[slot];
        if (out->controlled && out->frame == (long long)frame)
            return true;
    }
    if (hipMemcpy(out, K.rec.dev<WakeRecord>(p) + slot, sizeof *out, hipMemcpyDeviceToHost) != hipSuccess)
        return false;
    return out->controlled && out->frame == (long long)frame;
}
// Was leaf `id` parked in frame `frame`: a device result for a leaf under wake control, else the host's bookkeeping of
// sdrx_set_active.  Every answer the host gives about a parked frame comes through here.
bool leaf_parked_at(const sdrx_ctx *c, int id, unsigned long long frame)
{
    WakeRecord r;
    if (wake_record(c, id, frame, &r))
        return !r.active;
    return c->park.parked_at(id, frame);
}

// Leaf `id`'s payload of the delivered frame in host slot `slot`.  Option squelch: through the delivered directory -- a closed
// leaf has *len = 0 (the pointer is valid and not to be read).  Option park: so has a leaf that was parked in that frame.
const unsigned char *leaf_payload(const sdrx_ctx *c, int id, int slot, uint32_t *len)
{
    const Node &n = c->nodes[(size_t)id];
    *len = n.pay_len;
    if (leaf_parked_at(c, id, c->host_frame)) {
        *len = 0;
        return c->h_pay[slot];
    }
    if (!c->opt_squelch)
        return c->h_pay[slot] + n.pay_off;
    const size_t k = (size_t)c->sq.index[(size_t)id];
    const unsigned off = c->sq.offs[k];
    if (off == kSqClosed) {
        *len = 0;
        return c->h_pay[slot];
    }
    if (c->opt_preroll && c->sq.pre[k]) // the pre-rolled payload lies in front
        return c->h_pay[slot] + c->sq.hpack_off + 64 * ((size_t)off + c->sq.units[k]);
    return c->h_pay[slot] + c->sq.hpack_off + 64 * (size_t)off;
}
// Option preroll: leaf `id`'s payload of the frame BEFORE the delivered one, if the delivered frame carries it (else *len = 0)
const unsigned char *leaf_preroll(const sdrx_ctx *c, int id, int slot, uint32_t *len)
{
    *len = 0;
    if (!c->opt_preroll || leaf_parked_at(c, id, c->host_frame))
        return c->h_pay[slot];
    const size_t k = (size_t)c->sq.index[(size_t)id];
    if (c->sq.offs[k] == kSqClosed || !c->sq.pre[k])
        return c->h_pay[slot];
    *len = c->nodes[(size_t)id].pay_len;
    return c->h_pay[slot] + c->sq.hpack_off + 64 * (size_t)c->sq.offs[k];
}

// vfo::transmitData for every leaf, in the reference's order (vfo.cpp:426-453, sdrj.cpp:288-294)
void publish_all(sdrx_ctx *c, int slot)
{
    c->host_slot = slot;
    if (!c->cb)
        return;
    for (int i : c->publish_order) {
        const Node &n = c->nodes[(size_t)i];
        // USB leaves always publish; an IQ leaf only with a topic; ZmqPublisher::publish sends
        // nothing for len 0 (zmqpublisher.cpp:88) -- which is also what a leaf closed by option squelch has.
        uint32_t len = 0;
        const unsigned char *pay = leaf_payload(c, i, slot, &len);
        if (len == 0)
            continue;
        if (!n.d.demod_usb && n.d.topic[0] == 0)
            continue;
        char topic[5] = {0, 0, 0, 0, 0};
        for (int k = 0; k < 5 && n.d.topic[k]; ++k)
            topic[k] = n.d.topic[k];
        if (c->opt_preroll) { // a leaf that has just opened: the frame before, first
            uint32_t plen = 0;
            const unsigned char *pre = leaf_preroll(c, i, slot, &plen);
            if (plen)
                c->cb(c->cb_user, topic, n.rate, pre, plen);
        }
        c->cb(c->cb_user, topic, n.rate, pay, len);
    }
}

// How the payloads of the frame of parity p leave the device: two steps, and these two functions ARE them -- enqueue_frame (a
// frame that came through sdrx_submit*), start_owed_copy (sdrx_wait) and sdrx_fetch only choose the stream, what orders step 2
// behind step 1 (an event or a stream synchronisation), and when copy_owed is cleared.
//   1. queue_fixed_part (option squelch only): [meter_off, pay_bytes) of d_pay[p] -- meter records and directory -- which
//      always travels, behind the gate of the frame;
//   2. queue_payloads: with squelch the directory of step 1 must have ARRIVED in h_pay[p]: its packed_bytes says how much of
//      d_pack[p] goes to h_pay[p] + hpack_off, in ONE copy (none if every leaf is closed); without squelch the whole of d_pay[p].
// Both only read d_pay[p], d_pack[p] and the directory, whose next writer is frame f+2 (the safety argument above
// enqueue_frame, sdrx_frame.hip).
// Option watch: the records of the frame of parity p, part of what always travels -- the watch's, then the drift's and the band
// scan's of its sources, and option wake's of the controlled leaves (each: nothing before the first call that switched one on);
// option adc_meter's record of the frame's integer samples, the blanker's, the IQ balance's, the frequency shift's and the spur canceller's record (each: nothing with it off)
int queue_watch(sdrx_ctx *c, int p, hipStream_t st)
{
    for (const sdrx_ctx::Records *r : {&c->watch.rec, &c->drift.rec, &c->scan.rec, &c->wake.rec, &c->adc.rec, &c->bl.rec, &c->iq.rec, &c->sh.rec, &c->nt.rec})
        if (r->d[p])
            HIPCHK(c, hipMemcpyAsync(r->h[p], r->d[p], r->bytes(), hipMemcpyDeviceToHost, st));
    return SDRX_OK;
}
int queue_fixed_part(sdrx_ctx *c, int p, hipStream_t st)
{
    if (int rc = queue_watch(c, p, st))
        return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_pay[p] + c->meter_off, c->d_pay[p] + c->meter_off, c->pay_bytes - c->meter_off, hipMemcpyDeviceToHost, st));
    return SDRX_OK;
}
int queue_payloads(sdrx_ctx *c, int p, hipStream_t st)
{
    if (!c->opt_squelch) {
        if (int rc = queue_watch(c, p, st))
            return rc;
        HIPCHK(c, hipMemcpyAsync(c->h_pay[p], c->d_pay[p], c->pay_bytes, hipMemcpyDeviceToHost, st));
        return SDRX_OK;
    }
    SqHeader H;
    memcpy(&H, c->h_pay[p] + c->sq.dir_off, sizeof H);
    if (H.packed_bytes > c->sq.pack_bytes || H.packed_bytes % 64)
        return fail(c, SDRX_EHIP, "squelch: the directory of frame %lld names %llu packed bytes, the buffer holds %zu", H.frame,
                    H.packed_bytes, c->sq.pack_bytes);
    if (H.packed_bytes)
        HIPCHK(c, hipMemcpyAsync(c->h_pay[p] + c->sq.hpack_off, c->sq.d_pack[p], (size_t)H.packed_bytes, hipMemcpyDeviceToHost, st));
    c->sq.copied_slot[p] = H.packed_bytes;
    return SDRX_OK;
}
// Once the payloads are there too, the host's copy of the frame's directory: what sdrx_get_output, the callbacks,
// sdrx_get_squelch and sdrx_get_egress serve until the next delivery
void squelch_delivered(sdrx_ctx *c, int p)
{
    if (!c->opt_squelch)
        return;
    SqHeader H;
    const unsigned char *dir = c->h_pay[p] + c->sq.dir_off;
    memcpy(&H, dir, sizeof H);
    const size_t n = c->sq.offs.size();
    if (n) {
        memcpy(c->sq.offs.data(), dir + sizeof H, 4 * n);
        memcpy(c->sq.hang.data(), dir + sizeof H + 4 * n, 4 * n);
    }
    c->sq.n_open = H.n_open;
    c->sq.copied = c->sq.copied_slot[p];
    if (c->opt_preroll) {
        if (n)
            memcpy(c->sq.pre.data(), dir + sizeof H + 8 * n, 4 * n);
        c->sq.n_pre = (unsigned)H.pad[0];
        c->sq.pre_bytes = 0;
        for (size_t k = 0; k < n; ++k)
            if (c->sq.pre[k])
                c->sq.pre_bytes += 64ull * c->sq.units[k];
    }
    if (c->opt_squelch_auto && n) { // the threshold and the floor that decided this frame
        memcpy(c->sq.thr_eff.data(), dir + c->sq.aux_off, 8 * n);
        memcpy(c->sq.floor.data(), dir + c->sq.aux_off + 8 * n, 8 * n);
    }
}

// the oldest undelivered frame's payload copy, if sdrx_wait is the one to issue it (enqueue_frame: every frame under option
// squelch -- its directory has arrived by now -- and frames that carry the DC recurrence: the host waits for the frame's last
// kernel, then the copy goes out with nothing to wait for)
int start_owed_copy(sdrx_ctx *c)
{
    if (c->in_flight <= 0)
        return SDRX_OK;
    const int p = (int)((c->frame_no - (unsigned long long)c->in_flight) & 1ull);
    if (!c->copy_owed[p])
        return SDRX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t cs = p ? c->st.copy_stream2 : c->st.copy_stream;
    HIPCHK(c, hipEventSynchronize(c->opt_squelch ? c->sq.ev_dir[p] : c->st.ev_tail[p]));
    if (int rc = queue_payloads(c, p, cs))
        return rc;
    HIPCHK(c, hipEventRecord(c->st.ev_copied[p], cs));
    // only now: a wait retried after one of the calls above failed must find the copy still owed -- ev_copied[p] is still the
    // event of frame f - 2, which completed long ago, and h_pay[p] still holds THAT frame's payloads
    c->copy_owed[p] = false;
    return SDRX_OK;
}
// Fault injection for the hosts' error paths (tests/test_dropin_qt.py): SDRX_FAULT_WAIT=k makes the k-th sdrx_wait of the PROCESS
// fail like a HIP error does -- before the frame leaves the queue, and for good: every later frame call of that context fails
// too (HIP errors are sticky).  One shot per process, so that a host which recovers by building a new context gets a sound one.
bool injected_fault(sdrx_ctx *c, bool at_wait)
{
    static std::atomic<long> countdown{getenv("SDRX_FAULT_WAIT") ? atol(getenv("SDRX_FAULT_WAIT")) : 0};
    if (c->broken)
        return true;
    if (at_wait && countdown.load() > 0 && countdown.fetch_sub(1) == 1)
        c->broken = true;
    return c->broken;
}

// the oldest undelivered frame's payloads are in host memory afterwards (slot returned); no callbacks
int wait_frame(sdrx_ctx *c, int *slot)
{
    if (c->in_flight <= 0)
        return fail(c, SDRX_ESTATE, "sdrx_wait: no submitted frame is in flight");
    if (injected_fault(c, true))
        return fail(c, SDRX_EHIP, "sdrx_wait: injected fault (SDRX_FAULT_WAIT): the context is unusable from here on");
    int rc = start_owed_copy(c);
    if (rc)
        return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const unsigned long long f = c->frame_no - (unsigned long long)c->in_flight; // the oldest undelivered frame
    const int p = (int)(f & 1ull);
    HIPCHK(c, hipEventSynchronize(c->st.ev_copied[p]));
    c->in_flight--;
    c->host_slot = p;
    c->host_frame = f;
    squelch_delivered(c, p);
    if (c->in_flight == 0)
        drain_events(c);
    *slot = p;
    return SDRX_OK;
}

// The id list of a call that reads or sets per-leaf state: every id in range and a leaf, in list order; `once`: and listed once
// (the setters).  The whole list is checked before the caller writes or changes anything.
int check_leaf_ids(sdrx_ctx *c, const char *what, const int *ids, int n, bool once)
{
    std::vector<char> seen(once ? c->nodes.size() : 0, 0);
    for (int k = 0; k < n; ++k) {
        if (ids[k] < 0 || ids[k] >= (int)c->nodes.size())
            return fail(c, SDRX_EINVAL, "%s: bad vfo id %d", what, ids[k]);
        if (!c->nodes[(size_t)ids[k]].leaf)
            return fail(c, SDRX_EINVAL, "%s: vfo %d has children and publishes nothing (vfo.cpp:253-266)", what, ids[k]);
        if (once && seen[(size_t)ids[k]]++)
            return fail(c, SDRX_EINVAL, "%s: vfo %d listed twice", what, ids[k]);
    }
    return SDRX_OK;
}
// A delivered frame is on the host (c->host_slot, c->host_frame) for the getter `what`: frames queued with sdrx_process_device are
// brought over first (their payloads, records and directory).  `required` = false: a call that can answer without one.
int need_delivered(sdrx_ctx *c, const char *what, bool required = true)
{
    if (c->in_flight > 0 && c->host_slot < 0)
        return fail(c, SDRX_ESTATE, "%s: %d submitted frame(s), none delivered yet -- call sdrx_wait first", what, c->in_flight);
    if (c->pending_fetch)
        if (int rc = sdrx_fetch(c))
            return rc;
    if (required && c->host_slot < 0)
        return fail(c, SDRX_ESTATE, "%s: no frame has been delivered yet", what);
    return SDRX_OK;
}

// The checks every per-leaf call `what` shares, in the one order all of them keep (DESIGN.md "Per-leaf control calls"): handle,
// finalized, option `opt` (none: nullptr), list shape (`arrays`: every array that goes with `ids` is there), ids (in range, a
// leaf; listed once in a call that changes something), values (`bad(k)` says what is wrong with entry k), and what the call
// waits for.  A list of 0 entries passes with SDRX_OK like any other: the caller returns then.
enum LeafCall {
    kBetweenFrames, // changes state, or reads the device: no frame in flight
    kDelivered,     // reads the delivered frame: there is one (a list of 0 entries asks for none)
    kAnyTime,
};
const char *bad_switch(int32_t v) { return v == 0 || v == 1 ? nullptr : "the value must be 0 or 1"; }
const char *bad_auto(uint32_t ratio_q8, uint32_t window_frames) { return ratio_q8 > 0 && window_frames == 0 ? "window_frames 0 with a ratio" : nullptr; }
// sdrx_set_agc: what is wrong with a setting for a leaf that does (`usb`) or does not demodulate USB
const char *bad_agc(const sdrx_agc_cfg &a, bool usb)
{
    if (a.hi_ms == 0) // off for this leaf: the other fields are stored and ignored
        return nullptr;
    if (!(a.silent_ms <= a.lo_ms && a.lo_ms <= a.hi_ms && a.hi_ms <= (1u << 30)))
        return "the window needs silent_ms <= lo_ms <= hi_ms <= 2^30";
    if (!std::isfinite(a.up) || !std::isfinite(a.down) || !std::isfinite(a.gain_min) || !std::isfinite(a.gain_max))
        return "up, down, gain_min and gain_max must be finite";
    if (!(a.up >= 1.0f) || !(a.down > 0.0f && a.down <= 1.0f))
        return "the steps need up >= 1 and 0 < down <= 1";
    if (!(a.gain_min > 0.0f && a.gain_min <= a.gain_max))
        return "the limits need 0 < gain_min <= gain_max";
    if (!usb)
        return "the leaf does not demodulate USB: the gain does not act on a compress() leaf";
    return nullptr;
}
int leaf_call(sdrx_ctx *c, const char *what, int sdrx_ctx::*opt, const char *opt_name, const int *ids, bool arrays, int n, LeafCall mode,
              const std::function<const char *(int)> &bad = nullptr)
{
    if (!c)
        return SDRX_EINVAL;
    if (!c->finalized)
        return fail(c, SDRX_ESTATE, "%s before sdrx_finalize", what);
    if (opt && !(c->*opt))
        return fail(c, SDRX_ESTATE, "%s: option \"%s\" is off", what, opt_name);
    if (n < 0 || (n > 0 && (!ids || !arrays)))
        return fail(c, SDRX_EINVAL, "%s: n = %d, ids %p, or a null array beside them", what, n, (const void *)ids);
    if (int rc = check_leaf_ids(c, what, ids, n, mode == kBetweenFrames))
        return rc;
    for (int k = 0; bad && k < n; ++k)
        if (const char *why = bad(k))
            return fail(c, SDRX_EINVAL, "%s: vfo %d (entry %d): %s", what, ids[k], k, why);
    if (mode == kBetweenFrames && c->in_flight > 0)
        return fail(c, SDRX_ESTATE, "%s: %d submitted frame(s) not yet delivered -- call sdrx_wait first", what, c->in_flight);
    return mode == kDelivered && n > 0 ? need_delivered(c, what) : SDRX_OK;
}

// `count` entries of a job list into the device buffer `buf` (grown on demand), queued on the context's stream: the caller
// launches behind it and synchronises before `data` goes away.
template <class T>
int upload_jobs(sdrx_ctx *c, DevBuf<T> &buf, const void *data, size_t count)
{
    HIPCHK(c, buf.reserve(count));
    HIPCHK(c, hipMemcpyAsync(buf, data, sizeof(T) * count, hipMemcpyHostToDevice, c->st.stream));
    return SDRX_OK;
}

// A leaf's meter of one frame: its `n` records {sum_sq u64, clipped u32, peak u32} from record `first` of `rec` on, folded.
// (peak: magnitudes as bits -- the max of the bits is the max, a NaN wins)
struct MeterFold {
    uint64_t sum_sq = 0;
    uint32_t clipped = 0, peak = 0;
};
MeterFold fold_meter_records(const unsigned char *rec, int first, int n)
{
    MeterFold F;
    for (int j = 0; j < n; ++j) {
        const unsigned char *r = rec + 16 * (size_t)(first + j);
        uint64_t sum;
        uint32_t clipped, pk;
        memcpy(&sum, r, 8);
        memcpy(&clipped, r + 8, 4);
        memcpy(&pk, r + 12, 4);
        F.sum_sq += sum;
        F.clipped += clipped;
        F.peak = std::max(F.peak, pk);
    }
    return F;
}
} // namespace

extern "C" {

int sdrx_wait(sdrx_ctx *c)
{
    if (!c)
        return SDRX_EINVAL;
    int p = 0;
    const int rc = wait_frame(c, &p);
    if (rc)
        return rc;
    publish_all(c, p);
    return SDRX_OK;
}

int sdrx_fetch(sdrx_ctx *c)
{
    if (!c)
        return SDRX_EINVAL;
    if (!c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_fetch before sdrx_finalize");
    if (c->in_flight > 0)
        return fail(c, SDRX_ESTATE, "sdrx_fetch: %d submitted frame(s) not yet delivered -- call sdrx_wait", c->in_flight);
    if (c->frame_no == 0)
        return fail(c, SDRX_ESTATE, "sdrx_fetch: no frame processed yet");
    HIPCHK(c, hipSetDevice(c->device));
    const int p = (int)((c->frame_no - 1) & 1ull); // the last frame's payloads
    hipStream_t ts = c->opt_pipeline ? c->st.tail_stream : c->st.stream;
    if (int rc = pipeline_flush(c)) // frames still inside the software pipeline run to their end first
        return rc;
    if (c->pending_fetch && c->opt_squelch) { // the same two steps as sdrx_submit / sdrx_wait
        if (int rc = queue_fixed_part(c, p, ts))
            return rc;
        HIPCHK(c, hipStreamSynchronize(ts));
    }
    if (c->pending_fetch)
        if (int rc = queue_payloads(c, p, ts))
            return rc;
    int rc = drain(c);
    if (rc)
        return rc;
    if (c->pending_fetch)
        squelch_delivered(c, p);
    c->pending_fetch = false;
    c->host_frame = c->frame_no - 1;
    publish_all(c, p);
    return SDRX_OK;
}

int sdrx_get_output(sdrx_ctx *c, int id, const void **buf, uint32_t *len, uint32_t *rate)
{
    if (!c || id < 0 || id >= (int)c->nodes.size()) // (this call and sdrx_get_preroll: the id's range before anything else)
        return fail(c, SDRX_EINVAL, "bad vfo id %d", id);
    if (int rc = leaf_call(c, "sdrx_get_output", nullptr, nullptr, &id, true, 1, kAnyTime))
        return rc;
    if (int rc = need_delivered(c, "sdrx_get_output", buf != nullptr)) // (buf = NULL: a length query, good before any delivery)
        return rc;
    const Node &n = c->nodes[(size_t)id];
    uint32_t pay_len = n.pay_len;
    if (buf)
        *buf = leaf_payload(c, id, c->host_slot, &pay_len);
    else if (c->opt_squelch && c->host_slot >= 0)
        (void)leaf_payload(c, id, c->host_slot, &pay_len);
    if (len)
        *len = pay_len;
    if (rate)
        *rate = n.rate;
    return SDRX_OK;
}

int sdrx_get_meters(sdrx_ctx *c, const int *ids, int n, sdrx_meter *out)
{
    if (int rc = leaf_call(c, "sdrx_get_meters", &sdrx_ctx::opt_meter, "meter", ids, out != nullptr, n, kDelivered))
        return rc;
    if (n == 0)
        return SDRX_OK;
    const unsigned char *rec = c->h_pay[c->host_slot] + c->meter_off;
    for (int k = 0; k < n; ++k) {
        const Node &nd = c->nodes[(size_t)ids[k]];
        sdrx_meter m;
        memset(&m, 0, sizeof m);
        m.frame = (int64_t)c->host_frame;
        if (leaf_parked_at(c, ids[k], c->host_frame)) { // no value: nothing wrote the leaf's records in that frame
            out[k] = m;
            continue;
        }
        m.n_values = meter_n_values(nd);
        const MeterFold F = fold_meter_records(rec, nd.meter_first, nd.meter_n);
        m.sum_sq = F.sum_sq;
        m.clipped = F.clipped;
        memcpy(&m.peak, &F.peak, 4);
        out[k] = m;
    }
    return SDRX_OK;
}

// The whole list is checked before anything changes; then the software pipeline runs out with the old values, one upload of
// the job list, one k_squelch_set launch.
int sdrx_set_squelch(sdrx_ctx *c, const int *ids, const uint64_t *thr, const uint32_t *hang_frames, int n)
{
    if (int rc = leaf_call(c, "sdrx_set_squelch", &sdrx_ctx::opt_squelch, "squelch", ids, thr && hang_frames, n, kBetweenFrames))
        return rc;
    if (n == 0)
        return SDRX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    std::vector<SqJob> jobs((size_t)n);
    for (int k = 0; k < n; ++k)
        jobs[(size_t)k] = SqJob{thr[k], hang_frames[k], (unsigned)c->sq.index[(size_t)ids[k]]};
    if (int rc = upload_jobs(c, c->sq.d_jobs, jobs.data(), sizeof(SqJob) * jobs.size()))
        return rc;
    hipLaunchKernelGGL(k_squelch_set, dim3((n + 63) / 64), dim3(64), 0, c->st.stream, reinterpret_cast<const SqJob *>(c->sq.d_jobs.get()), n, c->sq.d_cfg, c->sq.d_hang);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->st.stream)); // (`jobs` lives on this stack)
    for (const SqJob &J : jobs) {
        c->sq.cfg[J.index] = SqCfg{J.thr, J.hang_frames, 0};
        c->sq.hang[J.index] = 0;
    }
    return SDRX_OK;
}

int sdrx_get_squelch(sdrx_ctx *c, const int *ids, int n, sdrx_squelch_state *out)
{
    if (int rc = leaf_call(c, "sdrx_get_squelch", &sdrx_ctx::opt_squelch, "squelch", ids, out != nullptr, n, kDelivered))
        return rc;
    for (int k = 0; k < n; ++k) {
        const size_t i = (size_t)c->sq.index[(size_t)ids[k]];
        sdrx_squelch_state s;
        memset(&s, 0, sizeof s);
        s.frame = (int64_t)c->host_frame;
        s.thr_sum_sq = c->sq.cfg[i].thr;
        s.hang_frames = c->sq.cfg[i].hang_frames;
        s.hang_left = c->sq.hang[i];
        s.open = c->sq.offs[i] != kSqClosed;
        out[k] = s;
    }
    return SDRX_OK;
}

// As sdrx_set_squelch: the whole list is checked before anything changes; then the software pipeline runs out with the old
// values, one upload of the job list, one k_squelch_set_auto launch (which restarts the named leaves' floor state).
int sdrx_set_squelch_auto(sdrx_ctx *c, const int *ids, const uint32_t *ratio_q8, const uint32_t *window_frames, int n)
{
    if (int rc = leaf_call(c, "sdrx_set_squelch_auto", &sdrx_ctx::opt_squelch_auto, "squelch_auto", ids, ratio_q8 && window_frames, n, kBetweenFrames,
                           [&](int k) { return bad_auto(ratio_q8[k], window_frames[k]); }))
        return rc;
    if (n == 0)
        return SDRX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    std::vector<SqAutoJob> jobs((size_t)n);
    for (int k = 0; k < n; ++k)
        jobs[(size_t)k] = SqAutoJob{ratio_q8[k], window_frames[k], (unsigned)c->sq.index[(size_t)ids[k]], 0};
    if (int rc = upload_jobs(c, c->sq.d_jobs, jobs.data(), sizeof(SqAutoJob) * jobs.size())) // (one buffer for both setters)
        return rc;
    hipLaunchKernelGGL(k_squelch_set_auto, dim3((n + 63) / 64), dim3(64), 0, c->st.stream, reinterpret_cast<const SqAutoJob *>(c->sq.d_jobs.get()), n,
                       c->sq.d_auto);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->st.stream)); // (`jobs` lives on this stack)
    for (const SqAutoJob &J : jobs)
        c->sq.acfg[J.index] = J;
    return SDRX_OK;
}

int sdrx_get_squelch_auto(sdrx_ctx *c, const int *ids, int n, sdrx_squelch_auto_state *out)
{
    if (int rc = leaf_call(c, "sdrx_get_squelch_auto", &sdrx_ctx::opt_squelch_auto, "squelch_auto", ids, out != nullptr, n, kDelivered))
        return rc;
    for (int k = 0; k < n; ++k) {
        const size_t i = (size_t)c->sq.index[(size_t)ids[k]];
        sdrx_squelch_auto_state s;
        memset(&s, 0, sizeof s);
        s.frame = (int64_t)c->host_frame;
        s.floor_valid = c->sq.floor[i] != kSqNone;
        s.floor_sum_sq = s.floor_valid ? c->sq.floor[i] : 0;
        s.thr_eff_sum_sq = c->sq.thr_eff[i];
        s.ratio_q8 = c->sq.acfg[i].ratio_q8;
        s.window_frames = c->sq.acfg[i].window_frames;
        out[k] = s;
    }
    return SDRX_OK;
}

// As sdrx_set_squelch_auto: the whole list is checked before anything changes; then the software pipeline runs out with the old
// settings, one upload of the job list, one k_agc_set launch (which restarts the named leaves' quiet_run).  A compress() leaf
// (hi_ms == 0: nothing else passes the check) has no slot on the device: its setting is stored on the host alone.
int sdrx_set_agc(sdrx_ctx *c, const int *ids, const sdrx_agc_cfg *cfgs, int n)
{
    if (int rc = leaf_call(c, "sdrx_set_agc", &sdrx_ctx::opt_agc, "agc", ids, cfgs != nullptr, n, kBetweenFrames,
                           [&](int k) { return bad_agc(cfgs[k], c->nodes[(size_t)ids[k]].d.demod_usb != 0); }))
        return rc;
    if (n == 0)
        return SDRX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = drain(c))
        return rc;
    std::vector<AgcJob> jobs;
    for (int k = 0; k < n; ++k) {
        const int slot = c->agc.slot[(size_t)ids[k]];
        if (slot < 0)
            continue;
        AgcJob J;
        memset(&J, 0, sizeof J);
        memcpy(&J.cfg, &cfgs[k], sizeof J.cfg);
        J.index = (unsigned)slot;
        jobs.push_back(J);
    }
    if (!jobs.empty()) {
        if (int rc = upload_jobs(c, c->agc.d_jobs, jobs.data(), jobs.size()))
            return rc;
        const int nj = (int)jobs.size();
        hipLaunchKernelGGL(k_agc_set, dim3((nj + 63) / 64), dim3(64), 0, c->st.stream, c->agc.d_jobs, nj, c->agc.d_cfg, c->agc.d_quiet);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->st.stream)); // (`jobs` lives on this stack)
    }
    for (int k = 0; k < n; ++k)
        c->agc.cfg[(size_t)ids[k]] = cfgs[k];
    return SDRX_OK;
}

int sdrx_get_agc(sdrx_ctx *c, const int *ids, int n, sdrx_agc_state *out)
{
    if (int rc = leaf_call(c, "sdrx_get_agc", &sdrx_ctx::opt_agc, "agc", ids, out != nullptr, n, kDelivered))
        return rc;
    if (n == 0)
        return SDRX_OK;
    const unsigned char *rec = c->h_pay[c->host_slot] + c->agc.rec_off;
    for (int k = 0; k < n; ++k) {
        sdrx_agc_state s;
        memset(&s, 0, sizeof s);
        s.frame = (int64_t)c->host_frame;
        s.cfg = c->agc.cfg[(size_t)ids[k]];
        const int slot = c->agc.slot[(size_t)ids[k]];
        if (slot < 0) { // a compress() leaf: the stored gain, which acts on nothing
            s.gain_used = s.gain_next = c->nodes[(size_t)ids[k]].d.gain;
        } else {
            AgcRecord R;
            memcpy(&R, rec + sizeof(AgcRecord) * (size_t)slot, sizeof R);
            s.gain_used = R.gain_used;
            s.gain_next = R.gain_next;
            s.action = R.action;
            s.quiet_run = R.quiet_run;
        }
        out[k] = s;
    }
    return SDRX_OK;
}

int sdrx_get_egress(sdrx_ctx *c, int64_t *frame, uint32_t *n_open, uint32_t *n_leaves, uint64_t *payload_bytes_copied)
{
    if (!c)
        return SDRX_EINVAL;
    if (!c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_get_egress before sdrx_finalize");
    if (c->host_slot < 0 || c->pending_fetch)
        return fail(c, SDRX_ESTATE, "sdrx_get_egress: no frame has been delivered yet (sdrx_wait / sdrx_fetch first)");
    const uint32_t leaves = (uint32_t)c->publish_order.size();
    if (frame)
        *frame = (int64_t)c->host_frame;
    if (n_leaves)
        *n_leaves = leaves;
    uint32_t n_active = leaves;
    for (int i : c->publish_order)
        n_active -= leaf_parked_at(c, i, c->host_frame);
    if (n_open)
        *n_open = c->opt_squelch ? c->sq.n_open : n_active;
    if (payload_bytes_copied)
        *payload_bytes_copied = c->opt_squelch ? c->sq.copied : (uint64_t)(c->meter_off ? c->meter_off : c->pay_bytes);
    return SDRX_OK;
}

int sdrx_get_preroll(sdrx_ctx *c, int id, const void **buf, uint32_t *len, int64_t *frame)
{
    if (!c || id < 0 || id >= (int)c->nodes.size())
        return fail(c, SDRX_EINVAL, "bad vfo id %d", id);
    if (int rc = leaf_call(c, "sdrx_get_preroll", &sdrx_ctx::opt_preroll, "preroll", &id, true, 1, kDelivered))
        return rc;
    uint32_t plen = 0;
    const unsigned char *pre = leaf_preroll(c, id, c->host_slot, &plen);
    if (buf)
        *buf = pre;
    if (len)
        *len = plen;
    if (frame)
        *frame = (int64_t)c->host_frame - 1;
    return SDRX_OK;
}

// Option adc_meter: the record of the delivered frame.  Whether that frame was measured is the host's note of the frame's
// parity (the slot of a frame that launched nothing holds an older frame's bytes).
int sdrx_get_adc_meter(sdrx_ctx *c, sdrx_adc_meter *out)
{
    if (!c)
        return SDRX_EINVAL;
    if (!c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_get_adc_meter before sdrx_finalize");
    if (!c->opt_adc_meter)
        return fail(c, SDRX_ESTATE, "sdrx_get_adc_meter: option \"adc_meter\" is off");
    if (!out)
        return fail(c, SDRX_EINVAL, "sdrx_get_adc_meter: null output pointer");
    if (int rc = need_delivered(c, "sdrx_get_adc_meter"))
        return rc;
    const int p = c->host_slot;
    const sdrx_ctx::Adc::Note &N = c->adc.note[p];
    memset(out, 0, sizeof *out);
    out->frame = (int64_t)c->host_frame;
    out->fmt = -1;
    if (N.fmt < 0 || N.frame != c->host_frame)
        return SDRX_OK;
    memcpy(out, c->adc.rec.host<AdcRecord>(p), sizeof *out);
    if (!out->measured || out->frame != (int64_t)c->host_frame || out->fmt != N.fmt)
        return fail(c, SDRX_EHIP, "sdrx_get_adc_meter: the record of frame %llu did not arrive (it names frame %lld)", c->host_frame, (long long)out->frame);
    return SDRX_OK;
}

int sdrx_get_preroll_count(sdrx_ctx *c, uint32_t *n_preroll, uint64_t *preroll_bytes)
{
    if (!c)
        return SDRX_EINVAL;
    if (!c->finalized)
        return fail(c, SDRX_ESTATE, "sdrx_get_preroll_count before sdrx_finalize");
    if (!c->opt_preroll)
        return fail(c, SDRX_ESTATE, "sdrx_get_preroll_count: option \"preroll\" is off");
    if (c->host_slot < 0 || c->pending_fetch)
        return fail(c, SDRX_ESTATE, "sdrx_get_preroll_count: no frame has been delivered yet (sdrx_wait / sdrx_fetch first)");
    if (n_preroll)
        *n_preroll = c->sq.n_pre;
    if (preroll_bytes)
        *preroll_bytes = c->sq.pre_bytes;
    return SDRX_OK;
}

} // extern "C"
