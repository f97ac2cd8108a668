// capi_run.hip -- run_stages: the one place that enqueues the stages of a run (pyramids, detection, LK, filter, triangulation,
// pose solve) on the context's streams, for the batch API, the lock-step loop and the drop-in calls alike; sync_all.
#include "capi_internal.h"

namespace vo_capi {

// The t1 pair a synchronous drop-in call deferred (vo_ctx::defer): staged and pulled over PCIe on stream `on`.
int flush_deferred(vo_ctx *c, hipStream_t on)
{
    const int n = c->defer.n;
    c->defer.n = 0;
    for (int k = 0; k < n; k++) {
        int rc = upload_image(c, c->defer.first + k, c->defer.img[k], c->defer.stride, hipMemcpyHostToDevice, /*idle*/ true, nullptr, -1, on);
        if (rc != VO_OK)
            return rc;
    }
    return VO_OK;
}

// The bucket grid and the image width VO_STAGE_DETECT can take; who / what: the caller's words for itself and for the stage.
int refuse_detect_shape(vo_ctx *c, const char *who, const char *what)
{
    if (!bucket_grid_ok(c->w, c->h, bucket_size(c), c->dprm.features_per_bucket))
        return fail(c, VO_ERR_ARG, (std::string(who) + ": bucket grid beyond the limits of the device bucketing (vo_hip.h, vo_detect_params)").c_str());
    if (c->w > 4096)
        return fail(c, VO_ERR_ARG, (std::string(who) + ": " + what + " handles images up to 4096 pixels wide").c_str());
    return VO_OK;
}

namespace {

// the timing events of the run: stage_events() says which pair brackets a stage
enum { PYR, DET, LK, FIL, TRI, PNP };

// what the parts of one run share (run_stages fills it in once)
struct Run {
    int stages;
    bool timed;
    hipEvent_t *evs;
    bool dry;   // lock-step loop, schedule probe: without the two kernels that advance a sequence's state
    bool split; // kept-pair call: hop 0 of LK before the t1 pair has arrived (run_lk)
    int wset;   // the set of DETECT / LK buffers this run writes
    bool serial;
    hipStream_t fs, ps, ts; // filter stream, pose stream, the stream the post-LK timing events go to
    vo_ctx::PoseBufs *pb;
    const int *seq_active;
    bool prep; // lock-step loop: pyramids (and, from vo_seq_step, FAST) on the prepare stream
};

int run_pyramids(vo_ctx *c, const Run &R)
{
    vo_ctx::Seq &sq = c->seq;
    hipStream_t pyrs = R.prep ? c->sel->prep : c->sel->stream;
    if (c->defer.n && !R.split) { // any run but the split one sends a deferred pair first, the old way
        int rcd = flush_deferred(c, c->sel->stream);
        if (rcd != VO_OK)
            return rcd;
    }
    if (R.timed)
        VO_HIP_TRY(c, hipEventRecord(R.evs[stage_events(PYR).start], pyrs));
    if (!R.split && (R.stages & VO_STAGE_PYRAMID)) { // (split: the t1 pyramids follow their pixels, in run_lk)
        const PyrImage *tab = c->d_imgs + c->pyr_first;
        const int ni = c->pyr_count;
        if (ni > 0) {
            // One launch per level, no LDS (round 4): a level is read once and gives its Scharr image, the next level and its
            // own border (pyramid.hip).  (Round 3: eight launches of three kernels that each fetched the level again.)
            launch_pyramid_fused(tab, ni, c->levels, c->lw, c->lh, c->lstride, pyrs);
            std::fill(c->img_stale.begin() + c->pyr_first, c->img_stale.begin() + c->pyr_first + ni, (uint8_t)0);
        }
    }
    if (R.prep)
        VO_HIP_TRY(c, hipEventRecord(sq.ev_pyr, pyrs));
    if (!sq.on && (R.stages & VO_STAGE_LK) && !R.split) { // (split: checked behind the deferred pyramids, in run_lk)
        for (int f = 0; f < c->n_frames; f++) {
            const Quad &q = c->h_quads[f];
            if (c->img_stale[q.l0] | c->img_stale[q.r0] | c->img_stale[q.l1] | c->img_stale[q.r1])
                return fail(c, VO_ERR_STATE, "vo_batch_run: VO_STAGE_LK on an image uploaded after its pyramid was last "
                                             "built (run VO_STAGE_PYRAMID over it first)");
        }
    }
    if (R.timed)
        VO_HIP_TRY(c, hipEventRecord(R.evs[stage_events(PYR).end], pyrs));
    return VO_OK;
}

int run_detect(vo_ctx *c, const Run &R)
{
    vo_ctx::Seq &sq = c->seq;
    const int B = c->n_frames, cap = c->cap, wset = R.wset;
    hipStream_t trk = c->sel->stream;
    if (R.stages & (VO_STAGE_DETECT | VO_STAGE_LK))
        VO_HIP_TRY(c, c->trk_free[wset].wait(trk));
    if (R.timed && !(R.stages & VO_STAGE_DETECT))
        VO_HIP_TRY(c, hipEventRecord(R.evs[stage_events(DET).start], trk));
    if (R.stages & VO_STAGE_DETECT) {
        const int bs = bucket_size(c), fpb = c->dprm.features_per_bucket;
        const int cells = (c->h / bs + 1) * (c->w / bs + 1);
        int rcr = refuse_detect_shape(c, "vo_batch_run", "VO_STAGE_DETECT");
        if (rcr != VO_OK)
            return rcr;
        const bool shi = shi_tomasi(c); // include/vo_detector.h: goodFeaturesToTrack in appendNewFeatures' one detector call
        if (shi && !sq.on) { // (the lock-step loop took its slots in vo_seq_configure)
            rcr = det_ensure(c, B);
            if (rcr != VO_OK)
                return rcr;
        }
        const bool fmask = fastmask_on(c); // include/vo_fast_mask.h: cv::FAST's call under the disc mask of the carried points
        if (fmask && !sq.on) {
            rcr = fm_ensure(c, B);
            if (rcr != VO_OK)
                return rcr;
        }
        // appendNewFeatures only when fewer than redetect_below features were carried in (visualOdometry.cpp:95)
        if (R.timed)
            VO_HIP_TRY(c, hipEventRecord(R.evs[stage_events(DET).start], trk));
        const int rp = sq.on ? (int)((sq.step - 1) % sq.ring) : 0; // ring slot of this step's t0 pair
        const bool ahead = R.prep && sq.have_corners[rp]; // its corners were detected one step ago on the prepare stream
        if (sq.on) {
            // the carried set lives on the device (seq_carry_kernel of the previous step wrote it on the filter stream)
            VO_HIP_TRY(c, sq.carry.wait(trk));
            // With look-ahead corners only their own signal is waited for; inline detection shares the FAST scratch buffers with
            // a look-ahead pass that may still run, and waits for every slot's
            for (int r2 = 0; r2 < sq.ring; r2++)
                if (r2 == rp || !ahead)
                    VO_HIP_TRY(c, sq.fast[r2].wait(trk));
            launch_seq_prepare(R.seq_active, c->d_ntracked, c->dprm.redetect_below, c->d_detect,
                               ahead && !topup_on(c) && !fmask ? sq.d_ncorn + (size_t)rp * sq.S : nullptr, c->d_nnew, B, trk);
            c->detect_uploaded = false;
        } else {
            bool changed = false;
            for (int f = 0; f < B; f++) {
                const int d = c->h_ntracked[f] < c->dprm.redetect_below ? 1 : 0;
                changed |= d != c->h_detect[f];
                c->h_detect[f] = d;
            }
            if (changed || !c->detect_uploaded) {
                VO_HIP_TRY(c, hipMemcpyAsync(c->d_detect, c->h_detect.data(), sizeof(int) * B, hipMemcpyHostToDevice, trk));
                VO_HIP_TRY(c, hipStreamSynchronize(trk)); // h_detect is reused by the next call
                c->detect_uploaded = true;
            }
        }
        int t = c->dprm.fast_threshold;
        t = t < 0 ? 0 : t > 255 ? 255 : t;
        const bool top = topup_on(c); // include/vo_topup.h: the detector's call under the disc mask of the carried points
        if (ahead && top) {
            // the look-ahead left the response maps of ring slot rp (seq_lookahead); seq_prepare_kernel above wrote the flags and,
            // given no counts, left d_nnew alone: discs, masked maximum, candidates and select run here under the flags, into the
            // detector's own list and d_nnew -- the inline route's buffers -- and the bucketing takes its split form
            int rcd = det_launch(c, c->quads_cur, c->d_detect, B, c->corn.d_pts, c->d_nnew, trk, sq.d_topmaps + (size_t)rp * sq.S * c->max_w * c->max_h);
            if (rcd != VO_OK)
                return rcd;
            launch_bucket(c->d_feat, c->corn.d_pts, c->d_fages, c->d_ntracked, c->d_nnew, c->fcap, c->w, c->h, bs, fpb, c->d_pts_det[wset],
                          c->d_ages_det[wset], c->d_npts_det[wset], cap, R.seq_active, c->d_overflow, B, trk);
        } else if (fmask) {
            // the unmasked list is the look-ahead's (ring slot rp; seq_prepare_kernel, given no counts, left d_nnew alone) or made
            // here into the record's own list; then the discs of the carried points, the filter under them -- which writes d_nnew,
            // 0 for a frame that does not detect again -- and the bucketing in its split form.  An unmasked list beyond fcap
            // arrives as fcap + 1 corners and leaves as the overflow flag.
            const float2 *raw = ahead ? sq.d_corners + (size_t)rp * sq.S * c->fcap : c->fm.d_raw;
            const int *n_raw = ahead ? sq.d_ncorn + (size_t)rp * sq.S : c->fm.d_nraw;
            if (!ahead)
                launch_fast_corners(c->d_imgs, c->quads_cur, c->d_detect, B, c->w, c->h, t, c->dprm.fast_nonmax, c->d_nmsmask, c->d_rowcnt, c->d_rowoff,
                                    nullptr, c->fm.d_nraw, c->fcap, c->fm.d_raw, trk);
            int rcd = fm_finish(c, c->d_detect, B, raw, n_raw, trk);
            if (rcd != VO_OK)
                return rcd;
            launch_bucket(c->d_feat, c->fm.d_filt, c->d_fages, c->d_ntracked, c->d_nnew, c->fcap, c->w, c->h, bs, fpb, c->d_pts_det[wset],
                          c->d_ages_det[wset], c->d_npts_det[wset], cap, R.seq_active, c->d_overflow, B, trk);
        } else if (ahead) {
            launch_bucket(c->d_feat, sq.d_corners + (size_t)rp * sq.S * c->fcap, c->d_fages, c->d_ntracked, c->d_nnew, c->fcap,
                          c->w, c->h, bs, fpb, c->d_pts_det[wset], c->d_ages_det[wset], c->d_npts_det[wset], cap, R.seq_active,
                          c->d_overflow, B, trk);
        } else if (shi) {
            // the corners in goodFeaturesToTrack's own order into the detector's list, their count -- 0 for a frame that does not
            // detect again, by the select pass itself -- into d_nnew, and the bucketing in its split form: no copy behind the
            // carried features.  A candidate list beyond fcap arrives as fcap + 1 corners and leaves as the overflow flag.
            int rcd = det_launch(c, c->quads_cur, c->d_detect, B, c->corn.d_pts, c->d_nnew, trk);
            if (rcd != VO_OK)
                return rcd;
            launch_bucket(c->d_feat, c->corn.d_pts, c->d_fages, c->d_ntracked, c->d_nnew, c->fcap, c->w, c->h, bs, fpb, c->d_pts_det[wset],
                          c->d_ages_det[wset], c->d_npts_det[wset], cap, R.seq_active, c->d_overflow, B, trk);
        } else {
            launch_detect_bucket(c->d_imgs, c->quads_cur, c->d_detect, B, c->w, c->h, t, c->dprm.fast_nonmax,
                                 c->d_nmsmask, c->d_rowcnt, c->d_rowoff, c->d_ntracked, c->d_nnew, c->fcap, c->d_feat, c->d_fages, bs, fpb,
                                 c->d_pts_det[wset], c->d_ages_det[wset], c->d_npts_det[wset], cap, R.seq_active,
                                 c->d_overflow, trk);
        }
        // (seq_enqueue_inputs: the NEXT step's PCIe ingest waits for this; under Shi-Tomasi so does this step's look-ahead pass,
        // seq_lookahead, which runs in the candidate buffers an inline detection has just used -- and, with the top-up on, behind
        // the masked passes of a step that ran on look-ahead maps too: they use those buffers on this stream)
        if (sq.on && (!R.prep || (shi && (!ahead || top))))
            VO_HIP_TRY(c, sq.detect.record(trk));
        c->pts_sel = wset;
        // the bucketed count is only known on the device; every later grid is sized by its bound
        const int bound = cells * fpb < cap ? cells * fpb : cap;
        c->max_pts_set = bound;
        c->pts_on_device = true;
    }
    if (R.timed)
        VO_HIP_TRY(c, hipEventRecord(R.evs[stage_events(DET).end], trk)); // (= start of LK)
    return VO_OK;
}

// A synchronous drop-in call on the kept pair that left its t1 pair in host memory (single_frame_setup): hop 0 of the LK
// chain reads the t0 pair only, so it starts before the t1 pair has crossed PCIe -- lk_hops_kernel [0, 1) on the tracking
// stream, the two pulls + the t1 pyramids on the idle filter stream beside it, lk_hops_kernel [1, 4) behind ev_t1_ready.
// Same bits as the one-launch chain (tests/test_kernel_emulation.py, the batch-against-call fuzz); the call gets shorter by
// what now hides under hop 0.  Any other run that finds a deferred pair sends it first, the old way (run_pyramids).
int run_lk(vo_ctx *c, const Run &R)
{
    vo_ctx::Seq &sq = c->seq;
    const int B = c->n_frames, cap = c->cap, wset = R.wset;
    hipStream_t trk = c->sel->stream;
    if (R.stages & VO_STAGE_LK) {
        if (R.prep) // the t1 pyramids of this step were built on the prepare stream
            VO_HIP_TRY(c, hipStreamWaitEvent(trk, sq.ev_pyr, 0));
        const LkParams lp = lk_params(c);
        if (R.split) {
            const Quad &q = c->h_quads[0];
            if (c->img_stale[q.l0] | c->img_stale[q.r0])
                return fail(c, VO_ERR_STATE, "synchronous call: the t0 pair has no pyramids");
            launch_lk_hops(c->d_imgs, c->quads_cur, cur_pts(c), cur_npts(c), cap, c->max_pts_set, B, c->d_trk2[wset],
                           c->d_status2[wset], lp, 0, 1, trk);
            hipStream_t side = c->sel->filter; // idle: the chain of a synchronous call stays on the tracking stream
            const int t1 = c->defer.first;
            int rcd = flush_deferred(c, side);
            if (rcd != VO_OK)
                return rcd;
            launch_pyramid_fused(c->d_imgs + t1, 2, c->levels, c->lw, c->lh, c->lstride, side);
            c->img_stale[t1] = c->img_stale[t1 + 1] = 0;
            VO_HIP_TRY(c, hipEventRecord(c->ev_t1_ready, side));
            VO_HIP_TRY(c, hipStreamWaitEvent(trk, c->ev_t1_ready, 0));
            if (c->img_stale[q.l1] | c->img_stale[q.r1])
                return fail(c, VO_ERR_STATE, "synchronous call: the t1 pair has no pyramids");
            launch_lk_hops(c->d_imgs, c->quads_cur, cur_pts(c), cur_npts(c), cap, c->max_pts_set, B, c->d_trk2[wset],
                           c->d_status2[wset], lp, 1, 4, trk);
        } else
            launch_lk_circular(c->d_imgs, c->quads_cur, cur_pts(c), cur_npts(c), cap, c->max_pts_set, B, c->d_trk2[wset],
                               c->d_status2[wset], lp, trk, &c->lk_queues);
        c->trk_last = wset;
        c->trk_next = wset ^ 1;
        if (sq.on) { // the ring slots holding this step's pairs may be overwritten once this LK has finished
            VO_HIP_TRY(c, sq.slot_free[(sq.step - 1) % sq.ring].record(trk));
            VO_HIP_TRY(c, sq.slot_free[sq.step % sq.ring].record(trk));
        }
    }
    if (R.timed)
        VO_HIP_TRY(c, hipEventRecord(R.evs[stage_events(LK).end], trk)); // end of LK on the tracking stream
    return VO_OK;
}

int run_filter_tri(vo_ctx *c, const Run &R)
{
    vo_ctx::Seq &sq = c->seq;
    vo_ctx::PoseBufs &pb = *R.pb;
    const int B = c->n_frames, cap = c->cap;
    const bool serial = R.serial;
    hipStream_t fs = R.fs, ts = R.ts;
    c->last_run_serial = serial;
    if (R.stages & (VO_STAGE_FILTER | VO_STAGE_TRIANGULATE | VO_STAGE_PNP)) {
        if (!serial) {
            VO_HIP_TRY(c, hipEventRecord(pb.ready, c->sel->stream));
            VO_HIP_TRY(c, hipStreamWaitEvent(fs, pb.ready, 0));
        }
        VO_HIP_TRY(c, pb.done.wait(fs)); // the pose solve of run k - 2 (same set)
    }
    if (R.timed)
        VO_HIP_TRY(c, hipEventRecord(R.evs[stage_events(FIL).start], ts));
    if (R.stages & VO_STAGE_FILTER) {
        launch_compact(cur_pts(c), c->d_trk2[c->trk_last], c->d_status2[c->trk_last], cur_npts(c), cap,
                       c->prm.consistency_threshold, c->d_outA, c->d_idxA, c->d_nA, pb.outB, pb.idxB, pb.nB, B, fs);
        if (sq.on) { // currentVOFeatures of every sequence after this frame (seq.hip)
            if (!R.dry)
                launch_seq_carry(R.seq_active, pb.outB, pb.nB, c->d_idxA, c->d_nA, cur_ages(c), cur_npts(c), cap, c->fcap,
                                 c->d_feat, c->d_fages, c->d_ntracked, c->d_overflow, sq.d_rows_carry, sq.d_nages, sq.d_info,
                                 sq.max_steps, B, fs);
            // (a dry run keeps the DEPENDENCY -- the next run's detection waits for this run's filter like it waits for
            // the carried features in a real step -- without the kernel that would advance the state)
            VO_HIP_TRY(c, sq.carry.record(fs));
        }
        if (!serial)
            VO_HIP_TRY(c, c->trk_free[c->trk_last].record(fs));
        // the points / ages this filter read belong to the OTHER set (a run without DETECT after a run with it):
        // the next DETECT into that set must wait for this filter too
        if (!serial && c->pts_sel >= 0 && c->pts_sel != c->trk_last)
            VO_HIP_TRY(c, c->trk_free[c->pts_sel].record(fs));
    }
    if (R.timed)
        VO_HIP_TRY(c, hipEventRecord(R.evs[stage_events(FIL).end], ts)); // (= start of triangulation)
    if (R.stages & VO_STAGE_TRIANGULATE) // stage-B rows: 0 = l0, 1 = r0, 2 = l1, 3 = r1
        launch_triangulate(c->d_P, c->d_P + 12, pb.outB, pb.outB + cap, (size_t)4 * cap, pb.nB, cap,
                           c->max_pts_set, B, pb.xyz, fs);
    if (R.timed)
        VO_HIP_TRY(c, hipEventRecord(R.evs[stage_events(TRI).end], ts)); // end of triangulation
    return VO_OK;
}

int run_pose(vo_ctx *c, const Run &R)
{
    vo_ctx::Seq &sq = c->seq;
    vo_ctx::PoseBufs &pb = *R.pb;
    const int B = c->n_frames, cap = c->cap;
    const bool serial = R.serial;
    hipStream_t fs = R.fs, ps = R.ps;
    if (!(R.stages & VO_STAGE_PNP)) {
        if (R.timed)
            VO_HIP_TRY(c, hipEventRecord(R.evs[stage_events(PNP).end], R.ts));
        return VO_OK;
    }
    if (!serial) {
        VO_HIP_TRY(c, hipEventRecord(pb.tri_done, fs));
        VO_HIP_TRY(c, hipStreamWaitEvent(ps, pb.tri_done, 0));
    }
    const PnpParams pp = pnp_params(c);
    if (c->prm.mono_rotation) {
        // rotation from the essential matrix of (pointsLeft_t0, pointsLeft_t1) = stage-B rows 0 and 2
        // (visualOdometry.cpp:146-157); the PnP solve below still provides the translation
        int rce = ensure_em(c);
        if (rce != VO_OK)
            return rce;
        // its own stream: the two chains only share their inputs, and together they would outlast the LK
        // launch they hide behind
        hipStream_t es = serial ? c->sel->stream : c->sel->em;
        if (!serial)
            VO_HIP_TRY(c, hipStreamWaitEvent(es, pb.tri_done, 0));
        // (crowded: the reduced-register variant of the essential-matrix kernels goes with the PnP one)
        launch_essential(pb.outB, pb.outB + 2 * cap, (size_t)4 * cap, pb.nB, cap, B, em_params(c), c->em, pb.em_results,
                         /*crowded*/ c->sched.waves >= 2, es);
        if (!serial)
            VO_HIP_TRY(c, hipEventRecord(pb.em_done, es));
    }
    launch_pnp_ransac(pb.xyz, pb.outB + 2 * cap, (size_t)4 * cap, pb.nB, cap, B, pp, pb.subsets, pb.models, pb.counts,
                      pb.rstate, c->sched.waves, ps, pb.epnp_ws, epnp_ws_frames(c), pb.epnp_gws, c->sched.wide, pb.rest_ws);
    if (c->prm.mono_rotation && !serial)
        VO_HIP_TRY(c, hipStreamWaitEvent(ps, pb.em_done, 0)); // `done` covers both chains; the tail below reads E's rotation
    SeqTail tail;
    // frame_pose is chained: step k integrates after step k - 1, whichever stream ran it -- only the refinement kernels of
    // consecutive chains are ordered, their RANSAC parts overlap.  (A dry run of the schedule probe keeps the ORDER without
    // the integration: with two pose streams its refinements otherwise overlap as no real step's can, and the probe saw
    // 0.34 ms per step where the loop then ran at 0.49 -- one sequence, profiles/r03_schedule_sweep.jsonl of r3_30.)
    // Not Signal::wait: this wait leaves the signal pending -- it is recorded again a few lines down in any case.
    if (sq.on && sq.integ.pending)
        VO_HIP_TRY(c, hipStreamWaitEvent(ps, sq.integ.ev, 0));
    if (sq.on && !R.dry) { // euler gates + integrateOdometryStereo of every sequence, one trajectory row each: inside
                           // select_refine_kernel (vo_seqtail.h)
        tail.active = R.seq_active;
        tail.em = c->prm.mono_rotation ? pb.em_results : nullptr;
        tail.pose = sq.d_pose;
        tail.traj = sq.d_traj;
        tail.info = sq.d_info;
        tail.n_rows = sq.d_rows;
        tail.max_steps = sq.max_steps;
    }
    launch_pnp_refine(pb.xyz, pb.outB + 2 * cap, (size_t)4 * cap, pb.nB, cap, B, pp, pb.models, pb.rstate, pb.inliers,
                      pb.results, c->sched.waves, tail, ps);
    if (sq.on)
        VO_HIP_TRY(c, sq.integ.record(ps));
    c->last_pose_stream = ps;
    if (R.timed)
        VO_HIP_TRY(c, hipEventRecord(R.evs[stage_events(PNP).end], ps)); // pose solve timed from the end of triangulation
    if (!serial) // (serial: whoever needs the results waits for the tracking stream)
        VO_HIP_TRY(c, pb.done.record(ps));
    return VO_OK;
}

} // namespace

// Which stream does what.  Pyramids, detection and LK run on the tracking stream (lock-step loop with the prepare stream: the
// pyramids there, one event ahead of LK).  Everything after LK is small, latency-bound work and leaves the tracking stream so
// that the next run's pyramid / LK launches overlap it:
//   filter stream: filter + triangulation of run k start as soon as LK(k) is done (they must not
//                  queue behind the pose solve of run k - 1, which is still running next to LK(k));
//   pose stream:   the PnP / RANSAC chain of run k (one stream, or one per buffer set: vo_ctx::sched.streams).
// Run k writes buffer set k % 2; its filter first waits for the pose solve of run k - 2 (same set).
// The tracking stream only waits -- before its next DETECT / LK, i.e. after a whole pyramid stage --
// for the filter to have consumed the points / tracks / status it is about to overwrite: DETECT and LK write the set of buffers
// (bucketed features / tracks + status) that the filter of two runs ago read; the filter of the previous run reads the other set.
// A synchronous drop-in call (vo_track_frame) has nothing to overlap with: everything on the tracking stream saves the
// three cross-stream hand-offs of the chain (~12 us each in the kernel timeline of one call).
// (serial: filter, triangulation and pose chain follow LK on the tracking stream itself -- stream order is the dependency,
// and none of the events that hand work from one stream to the next is recorded: each cost ~6 us of idle GPU between two
// kernels of the synchronous call, three of them per call, profiles/r04_track_frame_timeline.txt)
// dry (lock-step loop, schedule probe): everything but the two kernels that advance a sequence's state (seq_carry,
// seq_integrate) -- the step can then be repeated any number of times
int run_stages(vo_ctx *c, int stages, bool timed, hipEvent_t *evs, bool dry)
{
    if (c->n_images == 0)
        return fail(c, VO_ERR_STATE, "vo_batch_run before vo_batch_configure");
    if ((stages & (VO_STAGE_TRIANGULATE | VO_STAGE_PNP)) && !c->have_P)
        return fail(c, VO_ERR_STATE, "vo_batch_run: projection matrices not set");
    VO_HIP_TRY(c, hipSetDevice(c->device));
    (void)hipGetLastError(); // the launch check at the end must report THIS call's launches, not a stale error of the thread
    const vo_ctx::Seq &sq = c->seq;
    const bool touches_pose = (stages & (VO_STAGE_FILTER | VO_STAGE_TRIANGULATE | VO_STAGE_PNP)) != 0;
    Run R;
    R.stages = stages;
    R.timed = timed;
    R.evs = evs ? evs : c->ev;
    R.dry = dry;
    R.split = c->defer.n == 2 && !sq.on && c->n_frames == 1 && (stages & VO_STAGE_PYRAMID) && (stages & VO_STAGE_LK) &&
              !(stages & VO_STAGE_DETECT) && !c->tuning;
    R.wset = (stages & (VO_STAGE_DETECT | VO_STAGE_LK)) ? c->trk_next : c->trk_last;
    R.serial = c->serial_pose || (c->sync_call && !sq.on);
    const bool two_pose_streams = !R.serial && !c->prm.mono_rotation && c->sched.streams == 2;
    R.fs = R.serial ? c->sel->stream : c->sel->filter;
    R.ps = R.serial ? c->sel->stream : (two_pose_streams && (c->cur & 1)) ? c->sel->pnp2 : c->sel->pnp;
    R.ts = touches_pose ? R.fs : c->sel->stream;
    R.pb = &c->pb[c->cur];
    R.seq_active = sq.on ? sq.d_active + (size_t)(sq.step % VO_SEQ_INFLIGHT) * sq.S : nullptr;
    R.prep = sq.on && c->sched.prep;
    for (int (*part)(vo_ctx *, const Run &) : {run_pyramids, run_detect, run_lk, run_filter_tri, run_pose}) {
        int rc = part(c, R);
        if (rc != VO_OK)
            return rc;
    }
    VO_HIP_TRY(c, hipGetLastError());
    if (touches_pose) {
        c->last = c->cur;
        c->cur ^= 1;
    }
    return VO_OK;
}

// both streams idle (every getter and every synchronous entry point ends with this)
int sync_all(vo_ctx *c)
{
    VO_HIP_TRY(c, hipSetDevice(c->device));
    for (const StreamSlot &k : VO_STREAM_SLOTS) {
        if (k.role != INGEST || c->sel->*k.m) // (the ordinary set's ingest streams exist from their first use on)
            VO_HIP_TRY(c, hipStreamSynchronize(c->sel->*k.m));
        // while the partitioned twin is selected, the ordinary set's ingest streams are waited for all the same
        if (k.role == INGEST && c->sel != &c->streams.plain && c->streams.plain.*k.m)
            VO_HIP_TRY(c, hipStreamSynchronize(c->streams.plain.*k.m));
    }
    return VO_OK;
}

} // namespace vo_capi
