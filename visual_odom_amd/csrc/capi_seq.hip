// capi_seq.hip -- the lock-step sequence loop (vo_seq_*): the reference's frame loop (main.cpp:123-224) for S sequences at
// once, state carried on the device.
#include "capi_internal.h"

#include <sched.h>

#include <atomic>
#include <thread>

#include <algorithm>

namespace vo_capi {

void seq_free(vo_ctx *c)
{
    vo_ctx::Seq &q = c->seq;
    q.own.release();
    if (q.S && ingest_stream(c))
        (void)hipStreamSynchronize(ingest_stream(c)); // belongs to the context's stream set, not to the loop
    q = vo_ctx::Seq();
    c->cmp = vo_ctx::Compare(); // (its events were the loop's)
}

// The loop's signals are forgotten -- behind sync_all only -- in three groups, by what has been invalidated: SIG_STEP the end
// of every step (vo_seq_sync), SIG_INGEST what orders the ingest stream against the tracking stream (set_sched moves the
// ingest to another stream), SIG_CHAIN what one step hands to the next (vo_seq_reset(-1) forgets all three).  `detect` is in
// none: the ingest of the first step after a drain still waits for it, which costs one call and orders nothing.
void seq_forget(vo_ctx *c, int which)
{
    vo_ctx::Seq &q = c->seq;
    if (which & SIG_STEP)
        for (Signal &g : q.step_end)
            g.forget();
    if (which & SIG_INGEST) {
        for (int r = 0; r < VO_SEQ_MAX_RING; r++)
            q.slot_free[r].forget(), q.fast[r].forget();
        q.stage_free[0].forget(), q.stage_free[1].forget();
    }
    if (which & SIG_CHAIN)
        q.carry.forget(), q.integ.forget();
}

// a step failed after it had consumed its pairs, and part of it may be running: wait for the device, then refuse everything
// until the caller starts over -- the ring / staging slots of this step must not be rewritten under it
static int seq_step_failed(vo_ctx *c, int rc)
{
    const std::string why = c->err;
    (void)sync_all(c);
    c->err = why;
    c->seq.broken = true;
    return rc;
}

} // namespace vo_capi

extern "C" {

/* ---------------------------------- lock-step sequence loop -------------------------------- */

int vo_seq_configure(vo_ctx *c, int n_seq, int w, int h, int ring, int max_steps)
{
    if (!c)
        return VO_ERR_ARG;
    if (n_seq < 1 || n_seq > c->max_frames || ring < 2 || ring > VO_SEQ_MAX_RING || max_steps < 1 ||
        2 * ring * n_seq > c->max_images)
        return fail(c, VO_ERR_ARG, "vo_seq_configure: need 1 <= n_seq <= max_frames, ring 2 or 3, "
                                   "2 * ring * n_seq <= 6 * max_frames images");
    // image table: ring slot r holds the pairs [r][s] = images (r * S + s) * 2 + {0 left, 1 right}, so that the
    // pairs a step receives are one contiguous range for the pyramid stage
    int rc = vo_batch_configure(c, 2 * ring * n_seq, w, h, n_seq);
    if (rc != VO_OK)
        return rc;
    rc = sync_all(c);
    if (rc != VO_OK)
        return rc;
    seq_free(c);
    if (shi_tomasi(c)) { // (include/vo_detector.h) the detector's candidate buffers -- with the top-up of include/vo_topup.h on, the mask
                         // planes too --, one slot per sequence: here, never inside a step
        rc = det_ensure(c, n_seq);
        if (rc != VO_OK)
            return rc;
    }
    if (fastmask_on(c)) { // (include/vo_fast_mask.h) the planes and the lists of cv::FAST's mask, one slot per sequence: here as well
        rc = fm_ensure(c, n_seq);
        if (rc != VO_OK)
            return rc;
    }
    c->tf_base = -1; // the ring owns the image table (with ring 2 and one sequence the configure above changed nothing)
    // ONE sequence: the loop's two chains of small kernels on disjoint halves of the compute units (capi.hip,
    // ensure_partitioned_streams); more sequences fill the chip and want all of it
    rc = select_streams(c, n_seq == 1);
    if (rc != VO_OK)
        return rc;
    vo_ctx::Seq &q = c->seq;
    const size_t S = (size_t)n_seq;
    q.S = n_seq;
    q.ring = ring;
    q.max_steps = max_steps;
    // Prepare stream or plain copy stream?  Moving the pyramids and FAST off the tracking stream shortens a step's
    // critical path, which is what a SMALL number of sequences is bound by (round 2: 1 sequence 1.39 k -> 1.58 k frames/s,
    // 8 sequences 9.3 k -> 12.3 k); with many sequences the GPU is saturated, the step costs the sum of its kernels
    // either way and the extra concurrency only disturbs them (64 sequences 41.3 k -> 35.8 k, 256: 49.2 k -> 46.7 k).
    // Where the crossover lies depends on the image size and the point load, so it is part of the probed schedule: until
    // the first full step has been probed the loop runs WITH the prepare stream (so that the look-ahead corners the
    // prepare variant needs exist when the probe compares the two), unless this shape was probed before or is pinned.
    bool ok = true;
    {
        c->seq.on = true; // (for the key; seq_free below has cleared it)
        const TuneKey key = tune_key(c, VO_STAGE_ALL | VO_STAGE_DETECT);
        c->seq.on = false;
        vo_ctx::Schedule sc;
        const bool found = tuned_lookup(key, &sc);
        q.on = true;
        apply_pins(c, &sc);
        q.on = false;
        c->sched = sc;
        c->sched_probed = found && !all_pinned(c);
        if (found || all_pinned(c))
            memcpy(c->sched_key, key.k, sizeof(key.k));
        else
            c->sched_key[0] = -1; // the first full step probes
        ok = ensure_ingest_stream(c, sc.prep != 0) != nullptr;
    }
    Owner &o = q.own;
    ok = ok && o.device(&q.d_corners, (size_t)ring * S * c->fcap);
    ok = ok && o.device(&q.d_ncorn, (size_t)ring * S, /*zero*/ true);
    if (topup_on(c)) // (include/vo_topup.h) the look-ahead's response maps, one set per ring slot
        ok = ok && o.device(&q.d_topmaps, (size_t)ring * S * c->max_w * c->max_h);
    ok = ok && o.event(&q.ev_pyr);
    for (Signal &g : q.fast)
        ok = ok && o.signal(&g);
    ok = ok && o.device(&q.d_quads, (size_t)ring * S);
    ok = ok && o.device(&q.d_active, (size_t)VO_SEQ_INFLIGHT * S);
    ok = ok && o.pinned(&q.h_active, sizeof(int) * VO_SEQ_INFLIGHT * S, hipHostMallocDefault);
    ok = ok && o.device(&q.d_ing, (size_t)VO_SEQ_INFLIGHT * S);
    ok = ok && o.pinned(&q.h_ing, sizeof(SeqIngest) * VO_SEQ_INFLIGHT * S, hipHostMallocDefault);
    if (c->prm.rectify) { // (vo_ctx::Seq::d_raw; a loop without maps allocates none of this)
        ok = ok && o.device(&q.d_raw, c->rect_plane * 2 * S, /*zero*/ true);
        ok = ok && o.device(&q.d_ing_raw, (size_t)VO_SEQ_INFLIGHT * S);
        ok = ok && o.pinned(&q.h_ing_raw, sizeof(SeqIngest) * VO_SEQ_INFLIGHT * S, hipHostMallocDefault);
        ok = ok && o.device(&q.d_rect, (size_t)VO_SEQ_INFLIGHT * 2 * S);
        ok = ok && o.pinned(&q.h_rect, sizeof(RectImage) * VO_SEQ_INFLIGHT * 2 * S, hipHostMallocDefault);
    }
    ok = ok && o.device(&q.d_pose, S * 16);
    ok = ok && o.device(&q.d_traj, S * (size_t)max_steps * VO_SEQ_ROW);
    ok = ok && o.device(&q.d_info, S * (size_t)max_steps);
    ok = ok && o.device(&q.d_rows, S);
    ok = ok && o.device(&q.d_rows_carry, S);
    ok = ok && o.device(&q.d_nages, S);
    for (hipEvent_t *e : {&q.ev_upload, &q.detect.ev, &q.carry.ev, &q.integ.ev})
        ok = ok && o.event(e);
    for (Signal &g : q.slot_free)
        ok = ok && o.signal(&g);
    for (Signal &g : q.step_end)
        ok = ok && o.signal(&g);
    for (Signal &g : q.stage_free)
        ok = ok && o.signal(&g);
    for (auto &e : c->cmp.ev)
        ok = ok && o.event(&e, /*timing*/ true);
    if (!ok) {
        seq_free(c);
        (void)select_streams(c, false); // (n_seq == 1 had moved the context onto the CU-partitioned twin: not without a loop)
        return fail(c, VO_ERR_HIP, "vo_seq_configure: allocation failed");
    }
    std::vector<Quad> tab((size_t)ring * S);
    for (int r = 0; r < ring; r++)
        for (int s = 0; s < n_seq; s++) {
            const int a = (r * n_seq + s) * 2, b = (((r + 1) % ring) * n_seq + s) * 2;
            tab[(size_t)r * S + s] = Quad{a, a + 1, b, b + 1};
        }
    VO_HIP_TRY(c, hipMemcpy(q.d_quads, tab.data(), sizeof(Quad) * tab.size(), hipMemcpyHostToDevice));
    VO_HIP_TRY(c, hipMemset(q.d_info, 0, sizeof(SeqFrameInfo) * S * (size_t)max_steps));
    q.pushed.assign(S, 0);
    q.had_prev.assign(S, 0);
    q.ever.assign(S, 0);
    q.gap.assign(S, 0);
    q.h_rows.assign(S, 0);
    q.step = 0;
    q.on = true;
    return vo_seq_reset(c, -1);
}

int vo_seq_reset(vo_ctx *c, int seq)
{
    if (!c)
        return VO_ERR_ARG;
    vo_ctx::Seq &q = c->seq;
    if (!q.on)
        return fail(c, VO_ERR_STATE, "vo_seq_reset before vo_seq_configure");
    if (seq >= q.S)
        return fail(c, VO_ERR_ARG, "vo_seq_reset: bad sequence");
    if (q.begun && q.n_ing > 0 && !(q.broken && seq < 0))
        return fail(c, VO_ERR_STATE, "vo_seq_reset between vo_seq_push_pair and vo_seq_step");
    int rc = sync_all(c);
    if (rc != VO_OK)
        return rc;
    const int s0 = seq < 0 ? 0 : seq, s1 = seq < 0 ? q.S : seq + 1;
    double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int s = s0; s < s1; s++) {
        VO_HIP_TRY(c, hipMemcpy(q.d_pose + (size_t)s * 16, eye, sizeof(eye), hipMemcpyHostToDevice));
        q.pushed[s] = q.had_prev[s] = q.ever[s] = q.gap[s] = 0;
        q.h_rows[s] = 0;
    }
    if (seq < 0) {
        // everything is idle (sync_all above) and no sequence has a resident pair any more: the loop starts over -- ring
        // slot 0, event slot 0, all max_steps trajectory rows available again (a long-lived context that recycles its
        // sequences never runs out of steps)
        q.step = 0;
        sched_abandon(c); // (the dry probe's pick stays)
        q.begun = q.staged = q.broken = false;
        q.n_ing = 0;
        seq_forget(c, SIG_STEP | SIG_INGEST | SIG_CHAIN);
        for (auto &b : q.have_corners)
            b = false;
    }
    const size_t n = (size_t)(s1 - s0);
    VO_HIP_TRY(c, hipMemset(q.d_rows + s0, 0, sizeof(int) * n));
    VO_HIP_TRY(c, hipMemset(q.d_rows_carry + s0, 0, sizeof(int) * n));
    VO_HIP_TRY(c, hipMemset(q.d_nages + s0, 0, sizeof(int) * n));
    VO_HIP_TRY(c, hipMemset(c->d_ntracked + s0, 0, sizeof(int) * n));
    VO_HIP_TRY(c, hipMemset(c->d_fages + (size_t)s0 * c->fcap, 0, sizeof(int) * n * c->fcap));
    return VO_OK;
}

} // extern "C"

#define VO_SEQ_RUNAHEAD 3 // steps the host runs ahead of the device in the lock-step loop (seq_begin_step)

namespace vo_capi {

// First touch of the pending step (a push or the step call itself): its slot of the pinned per-step tables must
// have been consumed (step - VO_SEQ_INFLIGHT has finished), which also bounds the host's run-ahead.
int seq_begin_step(vo_ctx *c)
{
    vo_ctx::Seq &q = c->seq;
    if (q.begun)
        return VO_OK;
    VO_HIP_TRY(c, q.step_end[q.step % VO_SEQ_INFLIGHT].wait_host());
    // The host stays VO_SEQ_RUNAHEAD = 3 steps ahead of the device, not the VO_SEQ_INFLIGHT = 8 the per-step tables would allow
    // (late in round 6).  Found through the schedule comparison: a schedule whose pose chains cannot keep up with the tracking
    // stages fills a deep run-ahead with their backlog first and for ~50 steps reads as fast as its steps are issued (256
    // resident sequences: 1,1,1 measured 3.36 ms per step in its window, best of eight, and sustained 3.91).  And the deep
    // run-ahead itself costs throughput -- kernels of steps k + 2 ... k + 7 queued on every stream beside step k's: with the
    // schedule pinned (gpurun_out/r6_ra, 340 points, frames/s at 8 / 4 / 3 / 2 steps) 16 sequences 20.4 / 24.4 / 24.7 / 20.9 k,
    // 32: 31.8 / 35.5 / 36.2 / 29.5 k, 64: 50.0 / 49.9 / 56.9 / 41.5 k, 128: 71.5 / 71.0 / 73.6 / 55.2 k, 256: 76.0 / 76.6 / 76.3 /
    // 71.2 k, 256 from page-locked memory 50.9 / 51.1 / 51.4 / 45.8 k, 256 at 2 000 points 25.7 / 25.7 / 25.9 / 25.5 k; 8
    // sequences 12.7 k at 8 steps, 15.9 k at 3.  Pairs that come from HOST memory get one step more (the transfer of step k + 1
    // has to be under way while step k runs): 64 sequences from page-locked memory 41.8 / 42.0 / 38.7 k at 8 / 4 / 3 steps,
    // 8 sequences 12.4 / 14.6 / 14.4 k (gpurun_out/r6_ra2, r6_ra3).  (q.ing_pcie still describes the previous step here.)
    int ahead = q.ing_pcie ? VO_SEQ_RUNAHEAD + 1 : VO_SEQ_RUNAHEAD;
    if (dev_knob("VO_SEQ_RUNAHEAD", 0) > 0) // A/B: 1 .. 8
        ahead = dev_knob("VO_SEQ_RUNAHEAD", 0);
    if (ahead < VO_SEQ_INFLIGHT && q.step >= ahead)
        VO_HIP_TRY(c, q.step_end[(q.step - ahead) % VO_SEQ_INFLIGHT].wait_host());
    q.n_ing = 0;
    q.begun = true;
    return VO_OK;
}

// A push only records where the pair is; vo_seq_step moves all pairs of the step with ONE kernel on the copy stream
// (seq_ingest_kernel).  mode 0: pageable host memory, copied into the pinned staging area now so the caller's buffer
// is free on return; 1: page-locked host memory, read by the GPU over PCIe when the step runs; 2: device memory.
// a pageable image on its way into the pinned staging area (vo_seq_push_pairs copies a step's images with several threads)
struct StageCopy {
    uint8_t *dst;
    const uint8_t *src;
    int stride;
    int row_bytes = 0; // raw rows of a non-gray input format: bytes copied per row (0: gray, w) and the staging row pitch
    int dst_pitch = 0;
};
static void stage_copy(const StageCopy &k, int w, int h)
{
    if (k.row_bytes) {
        for (int y = 0; y < h; y++)
            memcpy(k.dst + (size_t)y * k.dst_pitch, k.src + (size_t)y * k.stride, (size_t)k.row_bytes);
        return;
    }
    if (k.stride == w)
        memcpy(k.dst, k.src, (size_t)w * h);
    else
        for (int y = 0; y < h; y++)
            memcpy(k.dst + (size_t)y * w, k.src + (size_t)y * k.stride, (size_t)w);
}

static int seq_push_impl(vo_ctx *c, int seq, const void *left, const void *right, int stride, int mode, std::vector<StageCopy> *defer)
{
    if (!c)
        return VO_ERR_ARG;
    vo_ctx::Seq &q = c->seq;
    if (!q.on)
        return fail(c, VO_ERR_STATE, "vo_seq_push_pair before vo_seq_configure");
    if (q.broken)
        return fail(c, VO_ERR_STATE, "vo_seq_push_pair: a previous vo_seq_step failed half-way; vo_seq_reset(ctx, -1) first");
    const int fmt = c->prm.input_format, bpp = ingest_bpp(fmt);
    if (seq < 0 || seq >= q.S || !left || !right || stride < c->w * bpp)
        return fail(c, VO_ERR_ARG, "vo_seq_push_pair: bad sequence / image / stride (at least w * bytes per pixel of vo_params.input_format)");
    if (q.pushed[seq])
        return fail(c, VO_ERR_STATE, "vo_seq_push_pair: this sequence already has a pair for the pending step");
    VO_HIP_TRY(c, hipSetDevice(c->device));
    int rc = seq_begin_step(c);
    if (rc != VO_OK)
        return rc;
    const int r = (int)(q.step % q.ring);
    SeqIngest e;
    e.stride = stride;
    e.image0 = (r * q.S + seq) * 2;
    if (mode == 0) {
        const int g = (int)(q.step & 1);
        const size_t img = (size_t)c->w * c->h * bpp; // (raw bytes: the ingest kernel converts)
        if (!q.h_stage || q.stage_img != img) {
            if (q.h_stage) {
                VO_HIP_TRY(c, hipStreamSynchronize(ingest_stream(c)));
                VO_HIP_TRY(c, q.own.give_back(&q.h_stage));
                VO_HIP_TRY(c, q.own.give_back(&q.d_stage));
            }
            q.stage_img = img;
            if (!q.own.pinned(&q.h_stage, img * 2 * 2 * (size_t)q.S, hipHostMallocDefault))
                return fail_hip(c, "vo_seq_push_pair: page-locked staging area", q.own.err);
            // the device twin serves the one-transfer path alone (seq_enqueue_inputs: from 32 sequences on); optional even
            // there: without it the kernel reads h_stage over PCIe
            if (q.S >= 32 && !q.own.device(&q.d_stage, img * 2 * 2 * (size_t)q.S))
                (void)hipGetLastError();
        }
        VO_HIP_TRY(c, q.stage_free[g].wait_host()); // the ingest kernel of step - 2 still reads this half of the staging area
        uint8_t *sl = q.h_stage + (((size_t)g * q.S + seq) * 2) * img, *sr = sl + img;
        const uint8_t *srcs[2] = {(const uint8_t *)left, (const uint8_t *)right};
        uint8_t *dsts[2] = {sl, sr};
        // an interleaved pair (VO_FMT_GRAY8_X2, right == left + 1) is ONE buffer: staged once, and still a pair the kernel reads once
        const bool one = fmt == VO_FMT_GRAY8_X2 && srcs[1] == srcs[0] + 1;
        for (int side = 0; side < (one ? 1 : 2); side++) {
            StageCopy k{dsts[side], srcs[side], stride};
            if (fmt != VO_FMT_GRAY8) {
                k.row_bytes = one ? 2 * c->w : (int)fmt_row_bytes(fmt, c->w);
                k.dst_pitch = c->w * bpp;
            }
            if (defer)
                defer->push_back(k); // (the caller copies the whole step's images at once, in parallel)
            else
                stage_copy(k, c->w, c->h);
        }
        e.left = sl;
        e.right = one ? sl + 1 : sr;
        e.stride = c->w * bpp;
        q.staged = true;
    } else if (mode == 1) {
        void *dl = nullptr, *dr = nullptr;
        if (hipHostGetDevicePointer(&dl, const_cast<void *>(left), 0) != hipSuccess ||
            hipHostGetDevicePointer(&dr, const_cast<void *>(right), 0) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, VO_ERR_ARG, "vo_seq_push_pair: host_pinned = 1 but the memory is not page-locked / mapped "
                                       "(hipHostMalloc, hipHostRegister, torch pin_memory)");
        }
        e.left = (const uint8_t *)dl;
        e.right = (const uint8_t *)dr;
    } else {
        e.left = (const uint8_t *)left;
        e.right = (const uint8_t *)right;
    }
    if (q.n_ing == 0) {
        q.ing_pcie = false;
        q.n_pageable = 0;
    }
    q.ing_pcie = q.ing_pcie || mode != 2;
    q.n_pageable += mode == 0;
    q.h_ing[(size_t)(q.step % VO_SEQ_INFLIGHT) * q.S + q.n_ing++] = e;
    q.pushed[seq] = 1;
    return VO_OK;
}

int seq_push(vo_ctx *c, int seq, const void *left, const void *right, int stride, int mode)
{
    return seq_push_impl(c, seq, left, right, stride, mode, nullptr);
}

} // namespace vo_capi

extern "C" {

int vo_seq_push_pair(vo_ctx *c, int seq, const uint8_t *left, const uint8_t *right, int stride, int host_pinned)
{
    return seq_push(c, seq, left, right, stride, host_pinned ? 1 : 0);
}

int vo_seq_push_pair_dev(vo_ctx *c, int seq, const void *left, const void *right, int stride)
{
    return seq_push(c, seq, left, right, stride, 2);
}

int vo_seq_push_pairs(vo_ctx *c, int n, const int32_t *seq_ids, const void *const *left, const void *const *right,
                      int stride, int kind)
{
    if (!c || n < 0 || (n > 0 && (!seq_ids || !left || !right)) || kind < 0 || kind > 2)
        return VO_ERR_ARG;
    // Pageable images are copied into the page-locked staging area before the call returns.  One thread moves ~30 GB/s: the
    // 239 MB of a 256-sequence KITTI step took 8 ms -- more than the step at the reference-default load (3.5 ms), and what
    // bounded that configuration at 31 k frames/s (gpurun_out/r6_ingab3).  From 16 images on the copies of a call are
    // spread over up to 8 threads (never more than the caller's affinity mask holds, one image at a time per thread).
    std::vector<StageCopy> copies;
    int rc = VO_OK;
    for (int i = 0; i < n && rc == VO_OK; i++)
        rc = seq_push_impl(c, seq_ids[i], left[i], right[i], stride, kind, kind == 0 ? &copies : nullptr);
    // (copies queued before a failing pair belong to pairs that were accepted: they are carried out all the same)
    if (!copies.empty()) {
        int cpus = (int)std::thread::hardware_concurrency();
#ifdef __linux__
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0)
            cpus = CPU_COUNT(&set);
#endif
        const int w = c->w, h = c->h;
        int nt = (int)copies.size() / 16;
        nt = nt > 8 ? 8 : nt;
        nt = nt > cpus ? cpus : nt;
        if (nt <= 1) {
            for (const StageCopy &k : copies)
                stage_copy(k, w, h);
        } else {
            std::atomic<size_t> next{0};
            auto work = [&]() {
                for (size_t i = next.fetch_add(1); i < copies.size(); i = next.fetch_add(1))
                    stage_copy(copies[i], w, h);
            };
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; t++)
                pool.emplace_back(work);
            work();
            for (std::thread &t : pool)
                t.join();
        }
    }
    return rc;
}

int vo_seq_step(vo_ctx *c)
{
    if (!c)
        return VO_ERR_ARG;
    vo_ctx::Seq &q = c->seq;
    if (!q.on)
        return fail(c, VO_ERR_STATE, "vo_seq_step before vo_seq_configure");
    if (!c->have_P)
        return fail(c, VO_ERR_STATE, "vo_seq_step: projection matrices not set");
    if (q.broken)
        return fail(c, VO_ERR_STATE, "vo_seq_step: a previous step failed half-way; vo_seq_reset(ctx, -1) first");
    // everything that can be refused is refused BEFORE the step consumes its pairs
    int rc = refuse_detect_shape(c, "vo_seq_step", "detection");
    if (rc != VO_OK)
        return rc;
    for (int s = 0; s < q.S; s++)
        if (q.pushed[s] && q.had_prev[s] && q.h_rows[s] >= q.max_steps) {
            // refuse the step and drop its pending pairs: the loop stays usable (trajectories can be read,
            // vo_seq_reset(s) gives the sequence its rows back)
            // Dropping a pair is a PAUSE of its sequence: if the caller moves on instead of re-pushing the same
            // pairs after vo_seq_reset(s), the next pair of such a sequence restarts its image pair (it is NOT matched against
            // the pair from two pushes ago) and the frame after that carries VO_SEQ_F_GAP, exactly like a resumed sequence.
            for (int k = 0; k < q.S; k++) {
                if (q.pushed[k])
                    q.had_prev[k] = 0;
                q.pushed[k] = 0;
            }
            q.begun = false;
            q.n_ing = 0;
            q.staged = false; // (the staging area holds only the dropped pairs: nothing was enqueued that reads it)
            return fail(c, VO_ERR_STATE, "vo_seq_step: a sequence's trajectory capacity (max_steps of vo_seq_configure) is "
                                         "exhausted; the pairs pushed for this step were dropped (re-push them after "
                                         "vo_seq_reset(seq), or go on: the affected sequences resume as after a pause)");
        }
    VO_HIP_TRY(c, hipSetDevice(c->device));
    rc = seq_begin_step(c);
    if (rc != VO_OK)
        return rc;
    const int slot = (int)(q.step % VO_SEQ_INFLIGHT);
    const int r = (int)(q.step % q.ring);
    // a sequence processes a frame iff it has a pair for this step and had one for the previous step.  A sequence that
    // RESUMES after steps without a pair restarts its image pair (this pair only builds pyramids) but keeps its carried
    // features and pose -- a case the reference's loop does not have; its next processed frame carries VO_SEQ_F_GAP
    // (active value 3) so that the missing transition is on record.
    int *act = q.h_active + (size_t)slot * q.S;
    int n_active = 0;
    for (int s = 0; s < q.S; s++) {
        const bool on = q.pushed[s] && q.had_prev[s];
        if (q.pushed[s] && !q.had_prev[s] && q.ever[s])
            q.gap[s] = 1;
        act[s] = on ? (q.gap[s] ? 3 : 1) : 0;
        if (on) {
            q.gap[s] = 0;
            q.h_rows[s]++;
        }
        n_active += on;
        q.ever[s] |= q.pushed[s];
        q.had_prev[s] = q.pushed[s];
        q.pushed[s] = 0;
    }
    q.n_active = n_active;
    rc = seq_enqueue_inputs(c, /*dry*/ false);
    if (rc != VO_OK) // (the step's bookkeeping is already consumed: same treatment as a failure further down)
        return seq_step_failed(c, rc);
    q.begun = false;
    c->pyr_first = r * q.S * 2;
    c->pyr_count = q.S * 2;
    int stages = VO_STAGE_PYRAMID;
    if (n_active > 0) {
        c->quads_cur = q.d_quads + (size_t)((q.step - 1) % q.ring) * q.S;
        stages |= VO_STAGE_DETECT | VO_STAGE_LK | VO_STAGE_FILTER | VO_STAGE_TRIANGULATE | VO_STAGE_PNP;
    }
    hipEvent_t *step_evs = &c->ring[(size_t)(q.step % VO_EVENT_SLOTS) * (VO_EV_PER_RUN)];
    rc = sched_before_step(c, stages, step_evs); // settles the schedule, or starts to (capi_sched.hip)
    if (rc == VO_OK)
        rc = run_stages(c, stages, true, step_evs);
    if (rc == VO_OK && !c->sched.prep)
        q.have_corners[r] = false; // the pair now in slot r has no look-ahead corners
    if (rc == VO_OK && c->sched.prep)
        rc = seq_lookahead(c, r);
    if (rc != VO_OK)
        return seq_step_failed(c, rc);
    // end of the step = end of its last stream: the pose stream when a frame was processed; without a processed frame
    // the step's work is the ingest + pyramids (+ FAST) -- on the prepare stream when there is one
    hipStream_t end_stream = n_active > 0 && c->last_pose_stream ? c->last_pose_stream : c->sched.prep ? c->sel->prep : c->sel->stream;
    VO_HIP_TRY(c, q.step_end[slot].record(end_stream));
    q.step++;
    return sched_after_step(c, end_stream); // a comparison of schedules over real steps counts this one
}

int vo_seq_sync(vo_ctx *c)
{
    if (!c)
        return VO_ERR_ARG;
    int rc = sync_all(c);
    if (rc == VO_OK)
        seq_forget(c, SIG_STEP);
    return rc;
}

int vo_seq_get_state(vo_ctx *c, int seq, float *pts, int *n_pts, int32_t *ages, int *n_ages, double *pose16)
{
    if (!c)
        return VO_ERR_ARG;
    vo_ctx::Seq &q = c->seq;
    if (!q.on)
        return fail(c, VO_ERR_STATE, "vo_seq_get_state before vo_seq_configure");
    if (seq < 0 || seq >= q.S)
        return fail(c, VO_ERR_ARG, "vo_seq_get_state: bad sequence");
    int rc = vo_seq_sync(c);
    if (rc != VO_OK)
        return rc;
    int np = 0, na = 0;
    VO_HIP_TRY(c, hipMemcpy(&np, c->d_ntracked + seq, sizeof(int), hipMemcpyDeviceToHost));
    VO_HIP_TRY(c, hipMemcpy(&na, q.d_nages + seq, sizeof(int), hipMemcpyDeviceToHost));
    if (pts && np > 0)
        VO_HIP_TRY(c, hipMemcpy(pts, c->d_feat + (size_t)seq * c->fcap, sizeof(float2) * np, hipMemcpyDeviceToHost));
    if (ages && na > 0)
        VO_HIP_TRY(c, hipMemcpy(ages, c->d_fages + (size_t)seq * c->fcap, sizeof(int) * na, hipMemcpyDeviceToHost));
    if (pose16)
        VO_HIP_TRY(c, hipMemcpy(pose16, q.d_pose + (size_t)seq * 16, sizeof(double) * 16, hipMemcpyDeviceToHost));
    if (n_pts)
        *n_pts = np;
    if (n_ages)
        *n_ages = na;
    return VO_OK;
}

int vo_seq_get_trajectory(vo_ctx *c, int seq, int first, int count, double *rows, int32_t *info, int *n_rows)
{
    if (!c)
        return VO_ERR_ARG;
    vo_ctx::Seq &q = c->seq;
    if (!q.on)
        return fail(c, VO_ERR_STATE, "vo_seq_get_trajectory before vo_seq_configure");
    if (seq < 0 || seq >= q.S || first < 0 || count < 0)
        return fail(c, VO_ERR_ARG, "vo_seq_get_trajectory: bad sequence / range");
    int rc = vo_seq_sync(c);
    if (rc != VO_OK)
        return rc;
    int n = 0;
    VO_HIP_TRY(c, hipMemcpy(&n, q.d_rows + seq, sizeof(int), hipMemcpyDeviceToHost));
    n = n < q.max_steps ? n : q.max_steps;
    if (n_rows)
        *n_rows = n;
    const int k = first + count <= n ? count : (first < n ? n - first : 0);
    static_assert(sizeof(SeqFrameInfo) == VO_SEQ_INFO * sizeof(int32_t), "SeqFrameInfo layout is the public info8 row");
    if (k > 0 && rows)
        VO_HIP_TRY(c, hipMemcpy(rows, q.d_traj + ((size_t)seq * q.max_steps + first) * VO_SEQ_ROW,
                                sizeof(double) * VO_SEQ_ROW * k, hipMemcpyDeviceToHost));
    bool ovf = false;
    if (k > 0) {
        std::vector<SeqFrameInfo> tmp((size_t)k);
        VO_HIP_TRY(c, hipMemcpy(tmp.data(), q.d_info + (size_t)seq * q.max_steps + first, sizeof(SeqFrameInfo) * k,
                                hipMemcpyDeviceToHost));
        for (const SeqFrameInfo &f : tmp)
            ovf |= f.overflow != 0;
        if (info)
            memcpy(info, tmp.data(), sizeof(SeqFrameInfo) * k);
    }
    if (ovf)
        return fail(c, VO_ERR_OVERFLOW, "vo_seq_get_trajectory: a frame's detection / bucketing exceeded the capacity "
                                        "given to vo_create (its result is truncated)");
    return VO_OK;
}

} // extern "C"
