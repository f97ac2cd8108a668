// capi_sched.hip -- the schedule of the pose chain next to the tracking stages: probe on the caller's data, pins, the
// per-process table of settled schedules and its export / import (vo_set_schedule, vo_get_schedule, vo_get_probe_log,
// vo_export_schedule, vo_import_schedule).
#include "capi_internal.h"

#include <algorithm>

namespace vo_capi {

static std::mutex g_tune_mu;
static std::map<TuneKey, vo_ctx::Schedule> g_tuned; // per process: a second context of the same shape starts tuned

bool tuned_lookup(const TuneKey &key, vo_ctx::Schedule *s)
{
    std::lock_guard<std::mutex> lk(g_tune_mu);
    auto it = g_tuned.find(key);
    if (it != g_tuned.end())
        *s = it->second;
    return it != g_tuned.end();
}
static void tuned_publish(const long long *k, const vo_ctx::Schedule &s)
{
    TuneKey key;
    memcpy(key.k, k, sizeof(key.k));
    std::lock_guard<std::mutex> lk(g_tune_mu);
    g_tuned[key] = s;
}

// The probe log (vo_ctx::probe_cand / probe_ms / probe_real / probe_n): where a schedule stands in it (-1: nowhere), and a time
// for it -- real = 1: measured over real steps of the lock-step loop -- which appends the schedule if the log has room
static int probe_log_find(const vo_ctx *c, const vo_ctx::Schedule &s)
{
    for (int i = 0; i < c->probe_n; i++)
        if (vo_ctx::Schedule::from(c->probe_cand[i]) == s)
            return i;
    return -1;
}
static void probe_log_record(vo_ctx *c, const vo_ctx::Schedule &s, float ms, int real)
{
    int i = probe_log_find(c, s);
    if (i < 0 && c->probe_n < VO_PROBE_LOG_MAX)
        c->probe_cand[i = c->probe_n++] = s.abi();
    if (i >= 0) {
        c->probe_ms[i] = ms;
        c->probe_real[i] = real;
    }
}

TuneKey tune_key(const vo_ctx *c, int stages)
{
    long long pts = c->max_pts_set;
    if (stages & VO_STAGE_DETECT) { // the bucketed count is only known on the device: its bound, like the launches
        const int bs = bucket_size(c);
        const long long cells = bs > 0 ? (long long)(c->h / bs + 1) * (c->w / bs + 1) : 1;
        pts = cells * c->dprm.features_per_bucket < c->cap ? cells * c->dprm.features_per_bucket : c->cap;
    }
    TuneKey key;
    key.k[0] = c->device;
    key.k[1] = c->seq.on ? 1 : 0;
    key.k[2] = c->w;
    key.k[3] = c->h;
    key.k[4] = c->levels;
    key.k[5] = c->n_frames;
    // (the synchronous drop-in call is keyed on the image shape only: a live sequence whose feature count drifts across a
    // bucket boundary must not pay a probe -- ~20 frame times -- in the middle of real-time use)
    key.k[6] = (c->sync_call && !c->seq.on) ? 0 : pts_bucket(pts);
    // (bit 5: the frame loop's detector -- a schedule probed under FAST is neither reused nor overwritten by a Shi-Tomasi context;
    // bit 6: its top-up under a mask of the carried points, include/vo_topup.h, likewise)
    key.k[7] = (c->prm.mono_rotation ? 1 : 0) | ((stages & VO_STAGE_DETECT) ? 2 : 0) | (c->sync_call && !c->seq.on ? 16 : 0) | (shi_tomasi(c) ? 32 : 0) |
               (topup_on(c) ? 64 : 0) | (fastmask_on(c) ? 128 : 0);
    return key;
}

// the four-kernel EPnP is a choice only for 5 .. VO_EPNP_WS_MAX_FRAMES frames per launch (pnp.hip, launch_pnp_ransac)
bool wide_knob_live(const vo_ctx *c)
{
    return c->n_frames > VO_EPNP_SPLIT_DEFAULT_FRAMES && c->n_frames <= VO_EPNP_WS_MAX_FRAMES && c->max_frames >= c->n_frames;
}

void apply_pins(const vo_ctx *c, vo_ctx::Schedule *s)
{
    if (c->pin.pose_waves)
        s->waves = c->pin.pose_waves;
    if (c->pin.pose_streams)
        s->streams = c->pin.pose_streams;
    if (c->pin.prepare >= 0)
        s->prep = c->pin.prepare;
    if (c->pin.epnp_wide_frames)
        s->wide = c->pin.epnp_wide_frames;
    if (!wide_knob_live(c))
        s->wide = 4; // (launches of <= 4 frames take the wide form anyway, launches of > 16 never: one value, no candidates)
    if (c->prm.mono_rotation)
        s->streams = 1; // the essential-matrix chain already runs next to the PnP chain on its own stream
    if (!c->seq.on)
        s->prep = 0;
}

bool all_pinned(const vo_ctx *c)
{
    return c->pin.pose_waves && (c->pin.pose_streams || c->prm.mono_rotation) && (!c->seq.on || c->pin.prepare >= 0) &&
           (!wide_knob_live(c) || c->pin.epnp_wide_frames);
}

// make `s` the schedule the next run uses.  Moving the lock-step loop's ingest between the plain copy stream and the
// prepare stream is only done with every stream idle (the ring slots, the FAST scratch buffers and the staging area are
// ordered per stream).
int set_sched(vo_ctx *c, const vo_ctx::Schedule &s)
{
    if (c->seq.on && (s.prep != c->sched.prep || !ingest_stream(c))) {
        int rc = sync_all(c);
        if (rc != VO_OK)
            return rc;
        if (!ensure_ingest_stream(c, s.prep != 0))
            return fail(c, VO_ERR_HIP, "could not create the copy stream");
        seq_forget(c, SIG_INGEST);
    }
    c->sched = s;
    return VO_OK;
}

// Resolve the schedule for the run that is about to be enqueued.  Returns 1 when this key has to be probed first
// (nothing cached, not everything pinned), 0 when c->sched is settled, < 0 on error.
int sched_resolve(vo_ctx *c, int stages)
{
    const TuneKey key = tune_key(c, stages);
    if (memcmp(key.k, c->sched_key, sizeof(key.k)) == 0)
        return 0;
    vo_ctx::Schedule s;
    const bool found = tuned_lookup(key, &s);
    if (!found && !all_pinned(c) && !c->serial_pose)
        return 1;
    apply_pins(c, &s);
    int rc = set_sched(c, s);
    if (rc != VO_OK)
        return rc;
    memcpy(c->sched_key, key.k, sizeof(key.k));
    c->sched_probed = found && !all_pinned(c);
    c->probe_n = 0; // this key was settled without a probe of this context: vo_get_probe_log must not show another key's
    return 0;
}

// What the pending step's kernels read that comes from the host: the pushed pairs -> ring slot step % ring with ONE
// kernel on the copy stream -- after the LK that still reads the slot's previous occupant (ring 2: the previous step's;
// ring 3: the one before, long finished), next to the previous step's kernels -- and the step's activity flags.
// dry (schedule probe): the same transfers again (same bytes to the same places), without the slot / staging bookkeeping.
int seq_enqueue_inputs(vo_ctx *c, bool dry)
{
    vo_ctx::Seq &q = c->seq;
    const int slot = (int)(q.step % VO_SEQ_INFLIGHT), r = (int)(q.step % q.ring);
    hipStream_t copy = ingest_stream(c);
    if (q.n_ing > 0) {
        if (!dry) // (a dry re-run writes the bytes the slot already holds, and leaves the signal to the real step)
            VO_HIP_TRY(c, q.slot_free[r].wait(copy));
        SeqIngest *d_tab = q.d_ing + (size_t)slot * q.S;
        SeqIngest *h_tab = q.h_ing + (size_t)slot * q.S;
        // Every sequence pushed a PAGEABLE pair: the step's half of the staging area is one contiguous block -- the copy engine
        // takes it across the link in one transfer (57 GB/s against the kernel's 48, and no shader wave, no L2 queue entry beside
        // LK: tools/ubench/ingest_under_load.hip), and the ingest kernel re-pitches it from its device twin, HBM to HBM.
        bool over_pcie = q.ing_pcie;
        // (from 32 sequences on: a transfer of a few megabytes is over before the copy's fixed cost is paid -- 8 sequences 0.70 ms
        // per step through the kernel, 0.80 through the engine; 64: 1.67 / 1.63; 256: 5.20 / 4.77 and, at 2 000 points, 11.34 / 10.28)
        if (q.d_stage && q.S >= 32 && q.n_pageable == q.S && q.n_ing == q.S) {
            const size_t half = q.stage_img * 2 * (size_t)q.S, off = (size_t)(q.step & 1) * half;
            VO_HIP_TRY(c, hipMemcpyAsync(q.d_stage + off, q.h_stage + off, half, hipMemcpyHostToDevice, copy));
            if (!dry) // (a dry re-run finds the entries already pointing at the device twin)
                for (int i = 0; i < q.n_ing; i++) {
                    h_tab[i].left = q.d_stage + (h_tab[i].left - q.h_stage);
                    h_tab[i].right = q.d_stage + (h_tab[i].right - q.h_stage);
                }
            over_pcie = false;
        }
        // A kernel that reads over PCIe starts behind the running step's DETECTION -- when the step can afford it.  Its host reads
        // park in the L2's queues, and the memory-bound kernels at the head of a step (pyramid pass, FAST, bucketing) pay for that
        // far more than LK does (256 sequences, page-locked pairs, 2 000 points: detection 0.99 ms beside the ingest against
        // 0.42 alone).  Measured with pinned schedules (gpurun_out/r6_ingwait): +1.5 .. +8 % where LK is long against the
        // transfer (2 000 points: 8.8 ms against 5), -3 .. -18 % where the step is the link's (340 points: 2.1 ms against 5 --
        // there every microsecond of the window counts).  So the wait is taken iff the LK of the newest step that has certainly
        // finished (VO_SEQ_INFLIGHT + 1 steps back, its stage events sit in the ring) lasted >= 1.6 x the transfer at 48 GB/s.
        // A heuristic on a schedule, never on a result.  (Not with the prepare stream: there the copy stream carries the step's
        // own pyramids.)
        bool wait_detect = false;
        if (over_pcie && !dry && q.step > VO_SEQ_INFLIGHT + 1) {
            hipEvent_t *old = &c->ring[(size_t)((q.step - VO_SEQ_INFLIGHT - 1) % VO_EVENT_SLOTS) * (VO_EV_PER_RUN)];
            float lk_ms = 0.f;
            const StageEvents lk = stage_events(2);
            if (hipEventQuery(old[lk.end]) == hipSuccess && hipEventElapsedTime(&lk_ms, old[lk.start], old[lk.end]) == hipSuccess)
                wait_detect = (double)lk_ms >= 1.6 * ((double)q.n_ing * 2.0 * c->w * c->h / 48e6);
            else
                (void)hipGetLastError(); // (a step without an LK stage left no such events)
        }
        if (dev_knob("VO_INGEST_WAIT", -1) >= 0) // A/B: 0 / 1 force
            wait_detect = dev_knob("VO_INGEST_WAIT", -1) != 0;
        if (wait_detect && over_pcie && !dry && !c->sched.prep)
            VO_HIP_TRY(c, q.detect.wait(copy));
        VO_HIP_TRY(c, hipMemcpyAsync(d_tab, h_tab, sizeof(SeqIngest) * q.n_ing, hipMemcpyHostToDevice, copy));
        // where the ingest kernel writes: the image table, or -- a context with maps -- the loop's raw planes, pair i to planes
        // 2 i, 2 i + 1 through a twin of the table; rectify_kernel then sends them to the ring slots the pairs were pushed for
        uint8_t *pix0 = c->d_pix + c->loff[0] + (size_t)VO_BY * c->lstride[0] + VO_BX;
        size_t img_bytes = c->img_bytes;
        int pitch = c->lstride[0];
        const SeqIngest *d_use = d_tab;
        if (c->prm.rectify) {
            SeqIngest *h_raw = q.h_ing_raw + (size_t)slot * q.S, *d_raw_tab = q.d_ing_raw + (size_t)slot * q.S;
            RectImage *h_rect = q.h_rect + (size_t)slot * 2 * q.S;
            for (int i = 0; i < q.n_ing; i++) { // (a dry re-run writes the values the tables already hold)
                h_raw[i] = h_tab[i];
                h_raw[i].image0 = 2 * i;
                for (int side = 0; side < 2; side++)
                    h_rect[2 * i + side] = RectImage{q.d_raw + (size_t)(2 * i + side) * c->rect_plane + rect_raw_origin(c->w), h_tab[i].image0 + side, side};
            }
            VO_HIP_TRY(c, hipMemcpyAsync(d_raw_tab, h_raw, sizeof(SeqIngest) * q.n_ing, hipMemcpyHostToDevice, copy));
            VO_HIP_TRY(c, hipMemcpyAsync(q.d_rect + (size_t)slot * 2 * q.S, h_rect, sizeof(RectImage) * 2 * q.n_ing, hipMemcpyHostToDevice, copy));
            pix0 = q.d_raw + rect_raw_origin(c->w);
            img_bytes = c->rect_plane;
            pitch = rect_raw_pitch(c->w);
            d_use = d_raw_tab;
        }
        if (c->prm.input_format == VO_FMT_GRAY8)
            launch_seq_ingest(d_use, q.n_ing, c->w, c->h, pitch, pix0, img_bytes, over_pcie, copy);
        else if (launch_seq_ingest_fmt(c->prm.input_format, d_use, q.n_ing, c->w, c->h, pitch, pix0, img_bytes, over_pcie, copy) != 0) // (ingest_fmt.hip: converts on the way)
            return fail(c, VO_ERR_STATE, "no converting kernel for this input format");
        if (c->prm.rectify)
            launch_rectify(q.d_rect + (size_t)slot * 2 * q.S, 2 * q.n_ing, c->w, c->h, pitch, c->d_rect_maps, c->lstride[0],
                           c->d_pix + c->loff[0] + (size_t)VO_BY * c->lstride[0] + VO_BX, c->img_bytes, copy);
        if (!dry && q.staged) {
            VO_HIP_TRY(c, q.stage_free[q.step & 1].record(copy));
            q.staged = false;
        }
    }
    if (!c->sched.prep) {
        VO_HIP_TRY(c, hipEventRecord(q.ev_upload, copy));
        VO_HIP_TRY(c, hipStreamWaitEvent(c->sel->stream, q.ev_upload, 0));
    }
    if (q.n_active > 0)
        VO_HIP_TRY(c, hipMemcpyAsync(q.d_active + (size_t)slot * q.S, q.h_active + (size_t)slot * q.S, sizeof(int) * q.S,
                                     hipMemcpyHostToDevice, c->sel->stream));
    return VO_OK;
}

// FAST + non-maximum suppression of the pairs in ring slot r (this step's new pairs), for the NEXT step's
// appendNewFeatures: on the prepare stream behind their pyramids (fast_score reads level 0 only), while this step's LK runs
int seq_lookahead(vo_ctx *c, int r)
{
    vo_ctx::Seq &q = c->seq;
    int t = c->dprm.fast_threshold;
    t = t < 0 ? 0 : t > 255 ? 255 : t;
    if (topup_on(c)) {
        // (include/vo_topup.h) the mask needs the carried set, which exists one step later; the response map does not: the map pass
        // alone, for every pair's left image, into ring slot r's maps.  The step's DETECT part finishes the call (run_detect)
        VO_HIP_TRY(c, q.detect.wait(ingest_stream(c)));
        int rc = det_lookahead_maps(c, q.d_quads + (size_t)r * q.S, q.S, q.d_topmaps + (size_t)r * q.S * c->max_w * c->max_h, ingest_stream(c));
        if (rc != VO_OK)
            return rc;
    } else if (shi_tomasi(c)) {
        // (include/vo_detector.h) goodFeaturesToTrack of every pair's left image into the ring slot's corner list, every frame
        // (which sequence detects again is known one step later: seq_prepare_kernel).  The candidate buffers are the ones an inline
        // detection of the step just enqueued may still use on the tracking stream: behind it.
        VO_HIP_TRY(c, q.detect.wait(ingest_stream(c)));
        int rc = det_launch(c, q.d_quads + (size_t)r * q.S, nullptr, q.S, q.d_corners + (size_t)r * q.S * c->fcap, q.d_ncorn + (size_t)r * q.S,
                            ingest_stream(c));
        if (rc != VO_OK)
            return rc;
    } else
        launch_fast_corners(c->d_imgs, q.d_quads + (size_t)r * q.S, nullptr, q.S, c->w, c->h, t, c->dprm.fast_nonmax,
                            c->d_nmsmask, c->d_rowcnt, c->d_rowoff, nullptr, q.d_ncorn + (size_t)r * q.S, c->fcap,
                            q.d_corners + (size_t)r * q.S * c->fcap, ingest_stream(c));
    VO_HIP_TRY(c, q.fast[r].record(ingest_stream(c)));
    q.have_corners[r] = true;
    VO_HIP_TRY(c, hipGetLastError());
    return VO_OK;
}

// one run of the probe: the stages, plus -- lock-step loop with the prepare stream -- the look-ahead detection a real
// step launches behind them (it recomputes the corners the real step will compute: idempotent)
int probe_run(vo_ctx *c, int stages, bool timed, hipEvent_t *evs, bool dry)
{
    int rc = dry && c->seq.on ? seq_enqueue_inputs(c, true) : VO_OK;
    if (rc == VO_OK)
        rc = run_stages(c, stages, timed, evs, dry);
    if (rc == VO_OK && dry && c->seq.on && c->sched.prep)
        rc = seq_lookahead(c, (int)(c->seq.step % c->seq.ring));
    return rc;
}

// STEADY-STATE milliseconds per run: n and n + K back-to-back runs are timed and the difference is divided by K, so that
// what every measurement has once -- the ramp-up and the last run's pose chain, which nothing overlaps -- cancels (timing
// one short burst instead favours the schedule with the shortest lone chain: the first version of this probe picked the
// 512-register kernels for 256 sequences, 10 % below the 256-register ones in the real loop).  K >= 20 ms of work, 6 .. 24.
// latency (the synchronous drop-in calls: one run, then the caller waits for it): the mean of K runs each followed by a
// synchronisation -- what such a caller sees; the steady-state figure hides exactly the chain latency it is waiting for.
int probe_candidate(vo_ctx *c, int stages, bool timed, hipEvent_t *evs, bool dry, bool latency, double *ms_per_run)
{
    using clk = std::chrono::steady_clock;
    if (latency) {
        int rc = sync_all(c);
        double total = 0;
        const int K = 8;
        for (int i = 0; i < K + 2 && rc == VO_OK; i++) {
            const auto t0 = clk::now();
            rc = probe_run(c, stages, timed, evs, dry);
            if (rc == VO_OK)
                rc = sync_all(c);
            if (i >= 2)
                total += std::chrono::duration<double, std::milli>(clk::now() - t0).count();
        }
        *ms_per_run = total / K;
        return rc;
    }
    auto burst = [&](int n, double *ms) {
        int rc = sync_all(c);
        const auto t0 = clk::now();
        for (int i = 0; i < n && rc == VO_OK; i++)
            rc = probe_run(c, stages, timed, evs, dry);
        if (rc == VO_OK)
            rc = sync_all(c);
        *ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
        return rc;
    };
    double warm = 0, ta = 0, tb = 0;
    int rc = burst(1, &warm);
    if (rc != VO_OK)
        return rc;
    int K = warm > 0 ? (int)ceil(20.0 / warm) : 24;
    K = K < 6 ? 6 : K > 24 ? 24 : K;
    rc = burst(3, &ta);
    if (rc == VO_OK)
        rc = burst(3 + K, &tb);
    if (rc != VO_OK)
        return rc;
    *ms_per_run = (tb - ta) / K;
    return VO_OK;
}

// Probe every candidate the pins leave open on the data the caller is about to process, keep the fastest.
// Batch mode: plain runs (a batch run is idempotent).  Lock-step loop: dry runs of the pending step.
int tune_schedule(vo_ctx *c, int stages, bool timed, hipEvent_t *evs, bool dry, bool latency, bool publish)
{
    const TuneKey key = tune_key(c, stages);
    // Candidates: every (waves, streams, prepare) the pins leave open with the four-kernel EPnP at its default reach -- at most
    // 2 x 2 x 2 -- and then, where that knob is live (5 .. 16 frames per run) and not pinned, the WINNER once more with the wide
    // reach: 8 + 1 candidates, not the 16 of the full product (that doubled the probe's cost beyond what vo_hip.h
    // states and filled the probe log to its last entry).
    static_assert(2 * 2 * 2 + 1 <= VO_PROBE_LOG_MAX, "the probe log holds every candidate");
    std::vector<vo_ctx::Schedule> cands;
    for (int waves = 1; waves <= 2; waves++)
        for (int streams = 1; streams <= (c->sync_call && !c->seq.on ? 1 : 2); streams++) // (a synchronous call runs on one stream)
            for (int prep = 1; prep >= 0; prep--) {
                vo_ctx::Schedule s, t;
                s.waves = waves;
                s.streams = streams;
                s.prep = prep;
                s.wide = c->pin.epnp_wide_frames && wide_knob_live(c) ? c->pin.epnp_wide_frames : VO_EPNP_SPLIT_DEFAULT_FRAMES;
                t = s;
                apply_pins(c, &t);
                if (!(t == s))
                    continue; // pinned away / not applicable
                if (prep && !c->seq.have_corners[c->seq.on ? (c->seq.step - 1) % c->seq.ring : 0])
                    continue; // no look-ahead corners for this step's t0 pair: the prepare variant cannot be shown
                cands.push_back(s);
            }
    if (cands.empty()) {
        vo_ctx::Schedule s;
        apply_pins(c, &s);
        cands.push_back(s);
    }
    bool probe_wide = wide_knob_live(c) && !c->pin.epnp_wide_frames;
    const bool measure = cands.size() > 1 || probe_wide;
    c->tuning = true;
    c->probe_n = 0;
    int rc = VO_OK, best = 0;
    double best_ms = 0;
    for (size_t i = 0; i < cands.size() && rc == VO_OK; i++) {
        rc = set_sched(c, cands[i]);
        double ms = 0;
        if (rc == VO_OK)
            rc = measure ? probe_candidate(c, stages, timed, evs, dry, latency, &ms) : VO_OK;
        if (rc == VO_OK && (i == 0 || ms < best_ms)) {
            best = (int)i;
            best_ms = ms;
        }
        probe_log_record(c, cands[i], (float)ms, 0);
        if (i + 1 == cands.size() && probe_wide && rc == VO_OK) {
            vo_ctx::Schedule wd = cands[best]; // the winner with the wide reach, once (appended: the loop runs it next)
            wd.wide = VO_EPNP_WS_MAX_FRAMES;
            cands.push_back(wd);
            probe_wide = false;
        }
    }
    c->tuning = false;
    if (rc != VO_OK)
        return rc;
    rc = set_sched(c, cands[best]);
    if (rc != VO_OK)
        return rc;
    // The per-process table (what a second context resolves from, what vo_export_schedule writes) only gets SETTLED schedules:
    // the lock-step loop's dry probe merely nominates -- its caller publishes after the comparison over real steps, or at once
    // when there is nothing to compare (the nominee used to be exported as if it were settled).
    if (publish)
        tuned_publish(key.k, cands[best]);
    memcpy(c->sched_key, key.k, sizeof(key.k));
    c->sched_probed = true;
    return VO_OK;
}

// run_stages for the batch entry points: settles the schedule first (cached, pinned or probed) when the run has a pose chain
// sync_call: a drop-in call that returns results -- the caller waits for every run, so candidates are compared by latency
int run_stages_auto(vo_ctx *c, int stages, bool timed, hipEvent_t *evs, bool sync_call)
{
    if (!c->tuning)
        c->sync_call = sync_call;
    if ((stages & VO_STAGE_PNP) && !c->tuning && c->n_images > 0 && c->have_P) {
        int need = sched_resolve(c, stages);
        if (need < 0)
            return need;
        if (need) {
            int rc = tune_schedule(c, stages, timed, evs, false, sync_call);
            if (rc != VO_OK)
                return rc;
        }
    }
    return run_stages(c, stages, timed, evs);
}

/* ------------------------ the lock-step loop's comparison of schedules over real steps ------------------------ */

// The comparison of schedules over real steps: untimed ramp steps behind a switch, and the shortest timed window.  3 and 12 until
// late in round 6 -- with 256 sequences fed from page-locked memory (a step that is the PCIe link's) such a window measured
// 5.14 ms per step for 2,2,0, which then sustains 5.7, against 5.17 for 1,1,0, which sustains 5.15; behind 10 ramp steps a
// 24-step window reads 5.3-5.5 against 5.05-5.2 (gpurun_out/r6_abwin): the chains of two pose streams take that long to
// overlap as they do sustained.
#define VO_AB_RAMP 10
#define VO_AB_MIN 24

// a step that shows the loop's real load (at least half of the sequences process a frame): only such steps settle and count
static bool real_load(const vo_ctx::Seq &q) { return q.n_active > 0 && 2 * q.n_active >= q.S; }

void sched_abandon(vo_ctx *c) // an unfinished comparison is dropped: the schedule in use (the dry probe's pick, or a pin) stays
{
    if (c->cmp.running())
        c->cmp.phase = 0;
}

// The dry runs leave out the two kernels that advance the state, and with them some of what the streams
// hide: measured against every pinned schedule (tools/schedule_sweep.py) their verdict on the prepare knob was
// wrong by 8-25 % at 1-32 sequences, and once the pose chain got shorter (round 3) they ranked the other two
// knobs wrongly by 5-8 % in five of sixteen loops (two pose streams look better dry than real with one
// sequence, one stream with 128).  So the dry probe only NOMINATES; up to four candidates then run for a while
// each over REAL steps and end-of-step GPU timestamps decide.  Returns false when there is nothing to compare.
static bool compare_start(vo_ctx *c)
{
    typedef vo_ctx::Schedule Schedule;
    vo_ctx::Compare &m = c->cmp;
    // The dry pick first (it stays if the loop ends before the comparison does).  Where the reach of the
    // four-kernel EPnP is a choice (5 .. 16 sequences) the dry pick with the OTHER reach comes second: dry, the two
    // differ by a per cent or two and the probe's choice between them is a coin flip, real steps differ by 17 %
    // at 8 sequences (0.54 against 0.65 ms per step, gpurun r5 `S=8` runs: 14.3 k or 12.0 k frames/s by that
    // flip).  Then one candidate per other (pose_streams, prepare) pair -- the two knobs the dry runs misjudge
    // -- each with the register budget the dry runs prefer for it, best dry time first, until four are named.
    int n = 0;
    m.list[n++] = c->sched;
    if (wide_knob_live(c) && !c->pin.epnp_wide_frames) {
        m.list[n] = c->sched;
        m.list[n].wide = c->sched.wide == VO_EPNP_WS_MAX_FRAMES ? VO_EPNP_SPLIT_DEFAULT_FRAMES : VO_EPNP_WS_MAX_FRAMES;
        n++;
    }
    int pairs[4], np = 0; // per other pair: its log entry with the best dry time
    for (int st = 1; st <= 2; st++)
        for (int pr = 1; pr >= 0; pr--) {
            Schedule pair;
            pair.streams = st, pair.prep = pr;
            if (pair.same_pair(c->sched))
                continue;
            int bi = -1;
            for (int i = 0; i < c->probe_n; i++)
                if (Schedule::from(c->probe_cand[i]).same_pair(pair) && (bi < 0 || c->probe_ms[i] < c->probe_ms[bi]))
                    bi = i;
            if (bi >= 0)
                pairs[np++] = bi;
        }
    std::sort(pairs, pairs + np, [&](int x, int y) { return c->probe_ms[x] < c->probe_ms[y]; });
    for (int k = 0; k < np && n < 4; k++) {
        m.list[n] = Schedule::from(c->probe_cand[pairs[k]]);
        // the reach of the four-kernel EPnP the dry probe preferred at ITS winner goes to every other nominee
        m.list[n++].wide = c->sched.wide;
    }
    if (n <= 1)
        return false;
    const int at = probe_log_find(c, c->sched);
    double ms = at >= 0 ? (double)c->probe_ms[at] : -1.0;
    ms = ms > 0.02 ? ms : 0.02;
    m.n = (int)ceil(25.0 / ms);
    m.n = m.n < VO_AB_MIN ? VO_AB_MIN : m.n > 48 ? 48 : m.n;
    m.cnt = n;
    m.extra = false;
    m.phase = 1;
    m.left = VO_AB_RAMP + m.n;
    memcpy(m.key, c->sched_key, sizeof(m.key));
    c->sched_probed = false; // "in progress" (vo_get_schedule reports 2)
    return true;
}

// Before a step of the lock-step loop is enqueued.  A step that shows the loop's real load settles the schedule: cached / pinned /
// probed with dry runs of THIS step -- everything but seq_carry and seq_integrate, so the step can be repeated; the probe's pick
// then either opens the comparison over real steps or, with nothing to compare, is the settled schedule and is published.
int sched_before_step(vo_ctx *c, int stages, hipEvent_t *evs)
{
    if (!real_load(c->seq) || c->tuning)
        return VO_OK;
    const int need = sched_resolve(c, stages);
    if (need <= 0)
        return need;
    int rc = tune_schedule(c, stages, true, evs, /*dry*/ true, /*latency*/ false, /*publish*/ false);
    if (rc == VO_OK && !(c->probe_n > 1 && compare_start(c)))
        tuned_publish(c->sched_key, c->sched);
    return rc;
}

// After the end event of a step (end_stream: the stream it was recorded on): counts the step, brackets the candidate's timed
// window, moves on to the next candidate, and behind the last one measures, selects, publishes and logs.
int sched_after_step(vo_ctx *c, hipStream_t end_stream)
{
    typedef vo_ctx::Schedule Schedule;
    vo_ctx::Compare &m = c->cmp;
    if (!m.running() || !real_load(c->seq))
        return VO_OK;
    const int ph = m.phase - 1;
    m.left--;
    if (m.left == m.n) // ramp over: the clock starts at the end of this step
        VO_HIP_TRY(c, hipEventRecord(m.ev[2 * ph], end_stream));
    if (m.left != 0)
        return VO_OK;
    VO_HIP_TRY(c, hipEventRecord(m.ev[2 * ph + 1], end_stream));
    int next = m.phase < m.cnt ? m.phase : -1; // the candidate the next window times
    int best = 0;
    float t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (next < 0) {
        VO_HIP_TRY(c, hipEventSynchronize(m.ev[2 * ph + 1]));
        for (int i = 0; i < m.cnt; i++) {
            VO_HIP_TRY(c, hipEventElapsedTime(&t[i], m.ev[2 * i], m.ev[2 * i + 1]));
            if (t[i] < t[best])
                best = i;
        }
    }
    // Round 6: every nominee ran with the register budget the DRY runs prefer for its (pose_streams, prepare) pair --
    // and at 64 sequences of 1241 x 376 they prefer the wrong one: 2,2,1 wins the comparison at 1.42 ms per step where
    // 1,2,1 runs 1.29 (45.2 k against 49.6 k frames/s, gpurun_out/r6_s64; the loop was bimodal by that pick).  So the
    // winner runs once more with the other budget before anything is settled -- from 32 sequences on: below, a window
    // of ~30 steps flatters the 256-register kernels (16 sequences: 0.76 ms per step in the window, 0.85 once the
    // pose stream's backlog has built up; 18.7 k frames/s where the untouched pick runs 20.9 k, gpurun_out/r6_twin).
    // ... and (later in round 6) so does the nominee of every other (pose_streams, prepare) pair, fastest pair first: with
    // 256 sequences of 340 points fed from page-locked memory the dry runs name 2,1,0 for the pair (1, 0) as often as
    // 1,1,0 -- it sustains 41 k frames/s where 1,1,0 sustains 49.5 k and everything with two pose streams 45 k
    // (gpurun_out/r6_pinsched), so the pair lost the comparison without its better half having run, and the loop was
    // bimodal by that.  (Every pair, not the best two or three: 2,1,0, 2,1,1 and 1,2,1 all measure 6.3 ms there, 0.01-0.03
    // apart -- gpurun_out/r6_ab2, r6_ab3.  From 32 sequences on the comparison is therefore exhaustive: all eight
    // schedules over real steps, ~34 steps each.)
    if (next < 0 && !m.extra && !c->pin.pose_waves && c->seq.S >= 32) {
        m.extra = true;
        int order[8], no = 0; // best nominee of every (pose_streams, prepare) pair, fastest pair first
        for (int i = 0; i < m.cnt; i++) {
            int k = 0;
            while (k < no && !m.list[order[k]].same_pair(m.list[i]))
                k++;
            if (k == no)
                order[no++] = i;
            else if (t[i] < t[order[k]])
                order[k] = i;
        }
        std::sort(order, order + no, [&](int a, int b) { return t[a] < t[b]; });
        const int first_new = m.cnt;
        for (int k = 0; k < no && m.cnt < 8; k++) {
            Schedule twin = m.list[order[k]];
            twin.waves = twin.waves == 1 ? 2 : 1;
            if (std::find(m.list, m.list + m.cnt, twin) == m.list + m.cnt)
                m.list[m.cnt++] = twin;
        }
        if (m.cnt > first_new)
            next = first_new;
    }
    if (next >= 0) {
        int rc = set_sched(c, m.list[next]); // (drains every stream first when the prepare knob changes)
        if (rc != VO_OK)
            return rc;
        m.phase++;
        m.left = VO_AB_RAMP + m.n;
        return VO_OK;
    }
    int rc = set_sched(c, m.list[best]);
    if (rc != VO_OK)
        return rc;
    tuned_publish(m.key, m.list[best]);
    for (int k = 0; k < m.cnt; k++) // the log shows what was measured over real steps (appended: a nominee the dry probe did
        probe_log_record(c, m.list[k], t[k] / m.n, 1); // not run in this form -- the wide reach)
    m.phase = m.cnt + 1;
    c->sched_probed = true;
    return VO_OK;
}

} // namespace vo_capi

extern "C" {

int vo_set_schedule(vo_ctx *c, const vo_schedule *s)
{
    if (!c)
        return VO_ERR_ARG;
    vo_schedule p = {0, 0, -1, 0};
    if (s)
        p = *s;
    if (p.epnp_wide_frames != 0 && p.epnp_wide_frames != VO_EPNP_SPLIT_DEFAULT_FRAMES && p.epnp_wide_frames != VO_EPNP_WS_MAX_FRAMES)
        return fail(c, VO_ERR_ARG, "vo_set_schedule: epnp_wide_frames 0 / 4 / 16");
    if (p.pose_waves < 0 || p.pose_waves == 3 || p.pose_waves > VO_DEV_MAX_POSE_WAVES || p.pose_streams < 0 || p.pose_streams > 2 ||
        p.prepare < -1 || p.prepare > 1)
        return fail(c, VO_ERR_ARG, "vo_set_schedule: pose_waves 0 / 1 / 2, pose_streams 0 / 1 / 2, prepare -1 / 0 / 1");
    int rc = sync_all(c);
    if (rc != VO_OK)
        return rc;
    c->pin = p;
    c->sched_key[0] = -1; // resolved again at the next run
    sched_abandon(c); // (a comparison over real steps in progress: the caller has just said what they want)
    if (c->seq.on) {      // the lock-step loop reads sched between steps: apply what is pinned now
        vo_ctx::Schedule sc = c->sched;
        apply_pins(c, &sc);
        rc = set_sched(c, sc);
    }
    return rc;
}

int vo_get_schedule(const vo_ctx *c, vo_schedule *cur, int *probed)
{
    if (!c || !cur)
        return VO_ERR_ARG;
    *cur = c->sched.abi();
    if (!c->seq.on)
        cur->prepare = 0;
    if (probed)
        *probed = (c->seq.on && c->cmp.running()) ? 2 : c->sched_probed ? 1 : 0;
    return VO_OK;
}

int vo_get_probe_log(const vo_ctx *c, vo_schedule *cands, float *ms, int *real, int *n)
{
    if (!c || !n)
        return VO_ERR_ARG;
    *n = c->probe_n;
    for (int i = 0; i < c->probe_n; i++) {
        if (cands)
            cands[i] = c->probe_cand[i];
        if (ms)
            ms[i] = c->probe_ms[i];
        if (real)
            real[i] = c->probe_real[i];
    }
    return VO_OK;
}

// The per-process table of settled schedules, out and in (a service must not pay up to 1.2 s of probing and
// three pipeline drains in every process).  A record = the key a schedule was settled for (device, mode, image size, pyramid
// levels, frames per run, point-load bucket, flags -- tune_key above) + the schedule.  Export after a warm-up run of each shape
// the service uses; import the records at start-up, before the first run: every context of the process then resolves those
// keys from the table (vo_get_schedule reports probed = 1) without running a single probe.  Records are plain data and stay
// valid for the same library build and device model; a key the table does not hold is probed as before.
int vo_export_schedule(vo_schedule_record *recs, int cap, int *n)
{
    if (!n || cap < 0 || (cap > 0 && !recs))
        return VO_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_tune_mu);
    int k = 0;
    for (const auto &kv : g_tuned) {
        if (k < cap) {
            for (int i = 0; i < 8; i++)
                recs[k].key[i] = kv.first.k[i];
            recs[k].schedule = kv.second.abi();
        }
        k++;
    }
    *n = k; // records in the table (may exceed cap: call again with a bigger array)
    return VO_OK;
}

int vo_import_schedule(const vo_schedule_record *recs, int n)
{
    if (n < 0 || (n > 0 && !recs))
        return VO_ERR_ARG;
    for (int k = 0; k < n; k++) { // validate everything before anything is taken over
        const vo_schedule &sc = recs[k].schedule;
        if ((sc.pose_waves != 1 && sc.pose_waves != 2 && !(sc.pose_waves == 4 && VO_DEV_MAX_POSE_WAVES == 4)) ||
            (sc.pose_streams != 1 && sc.pose_streams != 2) || (sc.prepare != 0 && sc.prepare != 1) ||
            (sc.epnp_wide_frames != VO_EPNP_SPLIT_DEFAULT_FRAMES && sc.epnp_wide_frames != VO_EPNP_WS_MAX_FRAMES) || recs[k].key[0] < 0 ||
            recs[k].key[2] < 32 || recs[k].key[3] < 32 || recs[k].key[4] < 1 || recs[k].key[4] > VO_MAX_LEVELS || recs[k].key[5] < 1)
            return VO_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(g_tune_mu);
    for (int k = 0; k < n; k++) {
        TuneKey key;
        for (int i = 0; i < 8; i++)
            key.k[i] = recs[k].key[i];
        g_tuned[key] = vo_ctx::Schedule::from(recs[k].schedule);
    }
    return VO_OK;
}

} // extern "C"
