// capi.hip -- host side of libvo_hip.so: context, device memory, streams, the batch API and its getters (C ABI declared in
// include/vo_hip.h).  No exceptions cross the ABI; every HIP failure becomes VO_ERR_HIP with a message retrievable through
// vo_last_error().  The other units of the ABI: capi_run.hip, capi_sched.hip, capi_seq.hip, capi_dropin.hip (capi_internal.h).
#include "capi_internal.h"

namespace vo_capi {

// pyramid geometry exactly as buildOpticalFlowPyramid: stop when the next level would not be
// larger than the 21 x 21 window (plan_depth)
int plan_levels(vo_ctx *c, int w, int h)
{
    const int levels = plan_depth(w, h, c->prm.lk_max_level) + 1;
    int cw = w, ch = h;
    size_t off = 0;
    for (int l = 0; l < levels; l++) {
        c->lw[l] = cw;
        c->lh[l] = ch;
        c->lstride[l] = level_stride(cw);
        c->loff[l] = off;
        off += (size_t)c->lstride[l] * (ch + 2 * VO_BY);
        off = (off + 255) / 256 * 256;
        cw = (cw + 1) / 2;
        ch = (ch + 1) / 2;
    }
    c->levels = levels;
    c->img_bytes = off;
    return 0;
}

// HIP streams of a context come from a per-device pool and go back to it in vo_destroy (they are never destroyed).
// Why: the runtime multiplexes a process's streams onto a few hardware queues in creation order, and which of a
// context's streams share a queue moves the latency-bound modes by 25 % (round-2 measurement: the SECOND vo_ctx of a
// process ran a one-sequence step in 0.80 instead of 0.63 ms).  A context created after another one was destroyed
// (bench.py's legs, a test session, a service that reconfigures) now gets the very same streams -- same mapping, same
// speed; contexts that are alive at the same time (one per host thread, examples/vo_multi_gpu.cpp) get a set each.
constexpr int VO_MAX_DEVICES = 64;
std::mutex g_pool_mu;
std::vector<StreamSet> g_pool[VO_MAX_DEVICES];
int g_pool_created[VO_MAX_DEVICES] = {};

bool acquire_streams(int device, StreamSet *out)
{
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        if (device < VO_MAX_DEVICES && !g_pool[device].empty()) {
            // the set that was created first: a process that only ever has one context alive always runs on the same streams
            size_t best = 0;
            for (size_t i = 1; i < g_pool[device].size(); i++)
                if (g_pool[device][i].id < g_pool[device][best].id)
                    best = i;
            *out = g_pool[device][best];
            g_pool[device].erase(g_pool[device].begin() + best);
            return true;
        }
    }
    StreamSet set;
    if (device < VO_MAX_DEVICES) {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        set.id = g_pool_created[device]++;
    }
    Streams &s = set.plain;
    bool ok = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess;
    // the post-LK streams carry a few hundred waves next to LK's hundred thousand: at equal priority
    // their kernels trickle in behind LK's workgroups (pose chain 1.1 ms alone, 5-10 ms next to LK) and
    // the next run ends up waiting for them, so they get the highest stream priority
    int least = 0, greatest = 0;
    ok = ok && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;
    ok = ok && hipStreamCreateWithPriority(&s.pnp, hipStreamNonBlocking, greatest) == hipSuccess;
    ok = ok && hipStreamCreateWithPriority(&s.pnp2, hipStreamNonBlocking, greatest) == hipSuccess;
    ok = ok && hipStreamCreateWithPriority(&s.filter, hipStreamNonBlocking, greatest) == hipSuccess;
    ok = ok && hipStreamCreateWithPriority(&s.em, hipStreamNonBlocking, greatest) == hipSuccess;
    *out = set;
    return ok;
}

// The lock-step loop's ingest stream (copy or prepare), created the first time a context of this set needs it.  Two flavours: the
// PREPARE stream has the highest priority (it carries the new pairs' pyramids and FAST besides the ingest kernel, short
// memory-bound kernels that have to find SIMD slots between the running step's LK waves); the plain COPY stream only
// carries the ingest kernel and keeps the default priority -- at the highest priority that kernel runs into the current
// step's pyramid / detection / LK kernels and costs each ~0.2 ms at 256 sequences (measured, round 3: 22.4 k -> 21.1 k
// frames/s).
hipStream_t ensure_ingest_stream(vo_ctx *c, bool prepare)
{
    hipStream_t &st = prepare ? c->sel->prep : c->sel->copy;
    if (st) // (the partitioned twin is created whole: always here)
        return st;
    int least = 0, greatest = 0;
    bool ok = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;
    ok = ok && (prepare ? hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest)
                        : hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) == hipSuccess;
    return ok ? st : nullptr;
}

// The PARTITIONED twin of a stream set (round 5): the post-LK streams get half of the GPU's compute units for themselves
// and the tracking / copy / prepare streams the other half (hipExtStreamCreateWithCUMask).  For ONE sequence in the
// lock-step loop: its step is two latency-bound chains of small kernels -- detection + LK of frame k + 1, the pose solve of
// frame k -- that otherwise land on the same CUs and slow each other (kernel trace of the loop: the refinement 152-162 us
// against 115 alone, bucketing 48 against 10, LK 230 against 200).  Measured (tools/cu_mask_ab.sh, pairs resident): 2 763 ->
// 3 115 frames/s with 128 + 128 CUs and two pose streams; 64 / 96 CUs for the pose side 3 014 / 2 978; with ONE pose stream
// the partition loses (1 445), and at 8 sequences it loses with any split (13.7 k -> 12.9 k): vo_seq_configure uses it for
// n_seq == 1 only and the schedule probe settles the rest.
bool ensure_partitioned_streams(StreamSet *s, int device)
{
    if (s->part_tried)
        return s->part.stream != nullptr;
    s->part_tried = true;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return false;
    const int n_cu = prop.multiProcessorCount, pose_cus = dev_knob("VO_POSE_CUS", n_cu / 2); // (developer build: 0 = no partition, n = CUs of the pose side)
    if (n_cu < 16 || n_cu > 1024 || pose_cus <= 0 || pose_cus >= n_cu)
        return false;
    std::vector<uint32_t> pose_mask((size_t)(n_cu + 31) / 32, 0u), trk_mask(pose_mask.size(), 0u);
    for (int cu = 0; cu < n_cu; cu++)
        (cu < pose_cus ? pose_mask : trk_mask)[(size_t)cu >> 5] |= 1u << (cu & 31);
    const uint32_t words = (uint32_t)pose_mask.size();
    Streams t;
    bool ok = true;
    for (const StreamSlot &k : VO_STREAM_SLOTS)
        ok = ok && hipExtStreamCreateWithCUMask(&(t.*k.m), words, (k.role == POST ? pose_mask : trk_mask).data()) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        for (const StreamSlot &k : VO_STREAM_SLOTS)
            if (t.*k.m)
                (void)hipStreamDestroy(t.*k.m);
        return false;
    }
    s->part = t;
    return true;
}

// which twin of its stream set a context enqueues on; the caller has drained every stream (sync_all)
int select_streams(vo_ctx *c, bool partitioned)
{
    // (no CU masks on this device / runtime: the ordinary set all the same)
    c->sel = partitioned && ensure_partitioned_streams(&c->streams, c->device) ? &c->streams.part : &c->streams.plain;
    c->last_pose_stream = nullptr;
    return VO_OK;
}

void release_streams(int device, const StreamSet &s)
{
    for (const Streams *t : {&s.plain, &s.part})
        for (const StreamSlot &k : VO_STREAM_SLOTS)
            if (t->*k.m)
                (void)hipStreamSynchronize(t->*k.m);
    if (!s.plain.stream || device >= VO_MAX_DEVICES)
        return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool[device].push_back(s);
}

} // namespace vo_capi

extern "C" {

void vo_default_params(vo_params *p)
{
    p->lk_max_level = 3;
    p->lk_max_count = 30;
    p->lk_epsilon = 0.01;
    p->lk_min_eig_threshold = 0.001;
    p->lk_full_chain = 0;
    p->consistency_threshold = 0;
    p->ransac_iterations = 500;
    p->ransac_reproj_error = 0.5f;
    p->ransac_confidence = (double)0.999f; // `float confidence = 0.999` in the reference
    p->mono_rotation = 0;                  // main.cpp:181 passes false
    p->em_prob = 0.999;                    // visualOdometry.cpp:152
    p->em_threshold = 1.0;                 // visualOdometry.cpp:152
    p->input_format = VO_FMT_GRAY8;
    p->rectify = 0; // (a vo_params is plain data: every rectification field is zero by default)
    p->rect_w = p->rect_h = p->rect_map_stride = 0;
    p->rect_map_x_left = p->rect_map_y_left = p->rect_map_x_right = p->rect_map_y_right = nullptr;
}

void vo_default_detect_params(vo_detect_params *p)
{
    p->fast_threshold = 20;     // feature.cpp:43
    p->fast_nonmax = 1;         // feature.cpp:44
    p->redetect_below = 2000;   // visualOdometry.cpp:95
    p->bucket_size = 0;         // 0 = rows / 10, visualOdometry.cpp:106
    p->features_per_bucket = 1; // visualOdometry.cpp:107
}

const char *vo_last_error(const vo_ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

void vo_destroy(vo_ctx *c)
{
    if (!c)
        return;
    (void)hipSetDevice(c->device);
    if (c->sel->stream)
        (void)sync_all(c); // nothing of this context may still run on streams that go back to the pool
    seq_free(c);
    c->own.release();
    release_streams(c->device, c->streams); // synchronises them; back to the per-device pool
    delete c;
}

vo_ctx *vo_create(int device, int max_w, int max_h, int max_pts, int max_frames)
{
    if (max_w < 32 || max_h < 32 || max_pts < 1 || max_frames < 1)
        return nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return nullptr;
    if (hipSetDevice(device) != hipSuccess)
        return nullptr;
    vo_ctx *c = new vo_ctx();
    c->device = device;
    c->max_w = max_w;
    c->max_h = max_h;
    c->cap = max_pts;
    c->max_frames = max_frames;
    c->max_images = 6 * max_frames; // 4 per frame for independent quads; 2 x ring (<= 3) per sequence of the lock-step loop
    vo_default_params(&c->prm);
    c->ransac_cap = 1000;
    const size_t B = (size_t)max_frames, cap = (size_t)max_pts;
    bool ok = acquire_streams(device, &c->streams);
    ok = ok && pnp_init_device(c->sel->stream) == 0;
    Owner &o = c->own;
    for (Signal &g : c->trk_free)
        ok = ok && o.signal(&g);
    ok = ok && o.event(&c->ev_t1_ready);
    // developer build: VO_SERIAL_POSE=1 enqueues the pose solve on the tracking stream (no overlap), so that a kernel trace shows
    // every kernel's stand-alone duration
    c->serial_pose = dev_knob("VO_SERIAL_POSE", 0) == 1;
    for (auto &e : c->ev)
        ok = ok && o.event(&e, /*timing*/ true);
    c->ring.assign((size_t)VO_EVENT_SLOTS * (VO_EV_PER_RUN), nullptr);
    for (auto &e : c->ring)
        ok = ok && o.event(&e, /*timing*/ true);
    // worst case pyramid bytes per image (5 levels, padded strides)
    {
        size_t per = 0;
        int cw = max_w, ch = max_h;
        for (int l = 0; l < VO_MAX_LEVELS; l++) {
            per += (size_t)level_stride(cw) * (ch + 2 * VO_BY) + 256;
            cw = (cw + 1) / 2;
            ch = (ch + 1) / 2;
        }
        c->pix_capacity = per * (size_t)c->max_images;
    }
    c->stage_slot = (size_t)level_stride(max_w) * max_h;
    c->stage_slot = (c->stage_slot + 255) / 256 * 256; // (slots stay 16-byte aligned for launch_pull_image)
    ok = ok && o.pinned(&c->h_stage, c->stage_slot * VO_STAGE_SLOTS, hipHostMallocMapped, &c->d_stage);
    ok = ok && o.pinned(&c->h_gather, frame_gather_bytes(c->cap), hipHostMallocMapped, &c->d_gather);
    ok = ok && o.pinned(&c->h_pts_stage, sizeof(float2) * (size_t)c->cap + 16, hipHostMallocMapped, &c->d_pts_stage);
    ok = ok && o.device(&c->d_pix, c->pix_capacity);
    ok = ok && o.device(&c->d_der, c->pix_capacity);
    ok = ok && o.device(&c->d_imgs, (size_t)c->max_images);
    ok = ok && o.device(&c->d_quads, B + VO_CONST_QUADS); // (the table + const_quad()'s four)
    ok = ok && o.device(&c->d_pts, B * cap);
    for (int k = 0; k < 2; k++) {
        ok = ok && o.device(&c->d_trk2[k], B * 4 * cap);
        ok = ok && o.device(&c->d_status2[k], B * 4 * cap);
    }
    ok = ok && o.device(&c->d_outA, B * 5 * cap);
    ok = ok && o.device(&c->d_npts, B, /*zero*/ true);
    ok = ok && o.device(&c->d_nA, B, /*zero*/ true);
    ok = ok && o.device(&c->d_idxA, B * cap);
    ok = ok && o.device(&c->d_P, (size_t)24);
    for (auto &b : c->pb) {
        ok = ok && o.device(&b.outB, B * 4 * cap);
        ok = ok && o.device(&b.nB, B, /*zero*/ true);
        ok = ok && o.device(&b.idxB, B * cap);
        ok = ok && o.device(&b.xyz, B * cap * 3);
        ok = ok && o.device(&b.subsets, B * c->ransac_cap * 5);
        ok = ok && o.device(&b.inliers, B * cap);
        ok = ok && o.device(&b.models, B * c->ransac_cap * 6);
        ok = ok && o.device(&b.counts, B * c->ransac_cap);
        ok = ok && o.device(&b.results, B);
        ok = ok && o.device(&b.rstate, B);
        ok = ok && o.device(&b.epnp_ws, (size_t)epnp_ws_frames(c) * VO_EPNP_WS_HYPS * VO_EPNP_WS_DOUBLES);
        ok = ok && o.device(&b.rest_ws, (size_t)epnp_ws_frames(c) * pnp_rest_ws_doubles(c->ransac_cap));
        if (VO_DEV_MAX_POSE_WAVES >= 4) // the slim pose chain's workspace (pnp.hip)
            ok = ok && o.device(&b.epnp_gws, B * VO_EPNP_GWS_BLOCKS * VO_EPNP_UT_DOUBLES * 64);
        ok = ok && o.event(&b.ready);
        ok = ok && o.signal(&b.done);
        ok = ok && o.event(&b.tri_done);
        ok = ok && o.event(&b.em_done);
    }
    vo_default_detect_params(&c->dprm);
    // carried + detected features of one frame before bucketing: cv::FAST on a textured image returns one corner
    // per ~20-40 pixels at most (non-maximum suppression leaves no two adjacent corners); beyond this capacity the
    // DETECT stage reports VO_ERR_OVERFLOW instead of silently bucketing a truncated list
    c->fcap = max_pts * 4 > 16384 ? max_pts * 4 : 16384;
    if ((long long)max_w * max_h / 16 > c->fcap)
        c->fcap = (int)((long long)max_w * max_h / 16);
    ok = ok && o.device(&c->d_nmsmask, B * (size_t)max_h * ((max_w + 63) / 64));
    ok = ok && o.device(&c->d_rowcnt, B * (size_t)max_h, /*zero*/ true);
    ok = ok && o.device(&c->d_rowoff, B * (size_t)max_h);
    ok = ok && o.device(&c->d_detect, B, /*zero*/ true);
    ok = ok && o.device(&c->d_ntracked, B, /*zero*/ true);
    ok = ok && o.device(&c->d_nnew, B, /*zero*/ true);
    ok = ok && o.device(&c->d_feat, B * (size_t)c->fcap);
    ok = ok && o.device(&c->d_fages, B * (size_t)c->fcap, /*zero*/ true);
    ok = ok && o.pinned(&c->h_feat_stage, features_stage_bytes(c->fcap), hipHostMallocMapped, &c->d_feat_stage);
    ok = ok && o.device(&c->d_ages, B * cap, /*zero*/ true);
    ok = ok && o.device(&c->d_overflow, B, /*zero*/ true);
    ok = ok && o.device(&c->lk_queues.d_next, (size_t)LKQ_WORDS, /*zero*/ true);
    for (int k = 0; k < 2; k++) {
        ok = ok && o.device(&c->d_pts_det[k], B * cap);
        ok = ok && o.device(&c->d_npts_det[k], B, /*zero*/ true);
        ok = ok && o.device(&c->d_ages_det[k], B * cap);
    }
    c->h_ntracked.assign(B, 0);
    c->h_detect.assign(B, 1);
    if (!ok) {
        vo_destroy(c);
        return nullptr;
    }
    c->h_npts.assign(B, 0);
    c->h_quads.assign(B, Quad{0, 0, 0, 0});
    c->img_stale.assign((size_t)c->max_images, 0);
    c->quads_cur = c->d_quads;
    if (hipMemcpy(c->d_quads + B, VO_CONST_QUAD_TABLE, sizeof(Quad) * VO_CONST_QUADS, hipMemcpyHostToDevice) != hipSuccess) {
        vo_destroy(c);
        return nullptr;
    }
    return c;
}

int vo_set_params(vo_ctx *c, const vo_params *p)
{
    if (!c || !p)
        return VO_ERR_ARG;
    if (p->lk_max_level < 0 || p->lk_max_level >= VO_MAX_LEVELS || p->ransac_iterations < 1 ||
        p->ransac_iterations > c->ransac_cap || !(p->ransac_confidence > 0 && p->ransac_confidence < 1) ||
        (p->mono_rotation && (!(p->em_prob > 0 && p->em_prob < 1) || !(p->em_threshold > 0))))
        return fail(c, VO_ERR_ARG, "vo_set_params: parameter out of range");
    if (p->input_format < VO_FMT_GRAY8 || p->input_format > VO_FMT_RGBA8)
        return fail(c, VO_ERR_ARG, "vo_set_params: input_format is not one of VO_FMT_*");
    // Rectification: fields identical to the context's own (off and off; or what vo_get_params returned, untouched) mean "the
    // maps I gave you" -- nothing is dereferenced, packed or reallocated.  Anything else is new maps: checked and packed now,
    // before anything of the context changes, committed below.
    const vo_params &q = c->prm;
    const bool rect_same = p->rectify == q.rectify &&
                           (!p->rectify || (p->rect_w == q.rect_w && p->rect_h == q.rect_h && p->rect_map_stride == q.rect_map_stride &&
                                            p->rect_map_x_left == q.rect_map_x_left && p->rect_map_y_left == q.rect_map_y_left &&
                                            p->rect_map_x_right == q.rect_map_x_right && p->rect_map_y_right == q.rect_map_y_right));
    std::vector<uint32_t> packed;
    if (!rect_same) {
        int rcr = rect_check_pack(c, p, &packed);
        if (rcr != VO_OK)
            return rcr;
    }
    // the staging slots of the synchronous calls hold RAW rows of a non-gray format: they grow when such a format is
    // configured (a gray context keeps what vo_create allocated) and never shrink
    const size_t raw = ((size_t)c->max_w * ingest_bpp(p->input_format) * c->max_h + 255) / 256 * 256;
    if (p->input_format != VO_FMT_GRAY8 && raw > c->stage_slot) {
        VO_HIP_TRY(c, hipSetDevice(c->device));
        int rcs = sync_all(c); // a queued pull may still read the old slots
        if (rcs != VO_OK)
            return rcs;
        uint8_t *h_new = nullptr, *d_new = nullptr;
        if (!c->own.pinned(&h_new, raw * VO_STAGE_SLOTS, hipHostMallocMapped, &d_new)) {
            const hipError_t e = c->own.err;
            (void)c->own.give_back(&h_new);
            return fail_hip(c, "vo_set_params: page-locked staging slots for this input format", e);
        }
        (void)c->own.give_back(&c->h_stage);
        c->h_stage = h_new;
        c->d_stage = d_new;
        c->stage_slot = raw;
        c->stage_next = 0;
    }
    if (!rect_same) {
        int rcr = rect_commit(c, p, packed);
        if (rcr != VO_OK)
            return rcr;
    }
    c->prm = *p;
    c->n_images = 0; // pyramid plan depends on lk_max_level: force re-configure
    return VO_OK;
}

int64_t vo_kept_pair_id(const vo_ctx *c) { return c && c->tf_base >= 0 ? c->tf_gen : 0; }

int vo_get_params(const vo_ctx *c, vo_params *p)
{
    if (!c || !p)
        return VO_ERR_ARG;
    *p = c->prm;
    return VO_OK;
}

int vo_batch_configure(vo_ctx *c, int n_images, int w, int h, int n_frames)
{
    if (!c)
        return VO_ERR_ARG;
    if (n_images < 1 || n_images > c->max_images || n_frames < 1 || n_frames > c->max_frames || w < 32 ||
        h < 32 || w > c->max_w || h > c->max_h)
        return fail(c, VO_ERR_ARG, "vo_batch_configure: size beyond the capacity given to vo_create");
    if (c->prm.rectify && (w != c->prm.rect_w || h != c->prm.rect_h))
        return fail(c, VO_ERR_ARG, "image size differs from vo_params.rect_w x rect_h: the context's rectification maps are for that size only");
    VO_HIP_TRY(c, hipSetDevice(c->device));
    if (c->cmask.any) { // every configuration drops the detector's masks (vo_corners_mask.h)
        VO_HIP_TRY(c, hipMemsetAsync(c->cmask.d_table, 0, sizeof(uint8_t *) * (size_t)c->max_images, c->sel->stream));
        std::fill(c->cmask.has.begin(), c->cmask.has.end(), 0);
        c->cmask.any = false;
    }
    if (c->seq.on) { // leaving the lock-step sequence loop: its steps may still be in flight
        int rcs = sync_all(c);
        if (rcs != VO_OK)
            return rcs;
        c->seq.on = false;
        (void)select_streams(c, false); // (the one-sequence loop runs on the partitioned streams)
        c->quads_cur = c->d_quads;
        c->n_images = 0; // force the full re-plan below
    }
    if (c->n_images == n_images && c->w == w && c->h == h && c->n_frames == n_frames) {
        c->pyr_first = 0; // a (re)configure always restores "build every pyramid"
        c->pyr_count = n_images;
        c->quads_cur = c->d_quads; // ... and "the quads are what vo_batch_set_quads last uploaded": a synchronous drop-in call
                                   // may have left the launches reading one of its constant quadruples
        return VO_OK;
    }
    c->sched_key[0] = -1; // a new shape: the schedule is resolved again at its first run
    c->tf_base = -1;      // (and the image table is laid out again)
    c->quads_cur = c->d_quads;
    plan_levels(c, w, h);
    if (c->img_bytes * (size_t)n_images > c->pix_capacity)
        return fail(c, VO_ERR_ARG, "vo_batch_configure: pyramid storage exceeds capacity");
    std::vector<PyrImage> tab((size_t)n_images);
    for (int i = 0; i < n_images; i++) {
        memset(&tab[i], 0, sizeof(PyrImage));
        for (int l = 0; l < c->levels; l++) {
            // pointers address pixel (0, 0); VO_BY rows and VO_BX columns of border precede it
            const size_t org = (size_t)i * c->img_bytes + c->loff[l] + (size_t)VO_BY * c->lstride[l] + VO_BX;
            tab[i].lvl[l] = c->d_pix + org;
            tab[i].der[l] = c->d_der + org;
            tab[i].w[l] = c->lw[l];
            tab[i].h[l] = c->lh[l];
            tab[i].stride[l] = c->lstride[l];
        }
    }
    VO_HIP_TRY(c, hipMemcpyAsync(c->d_imgs, tab.data(), sizeof(PyrImage) * n_images, hipMemcpyHostToDevice,
                                 c->sel->stream));
    // the Scharr border is BORDER_CONSTANT 0 (and stays 0: scharr_kernel writes interiors only)
    VO_HIP_TRY(c, hipMemsetAsync(c->d_der, 0, sizeof(uint32_t) * c->img_bytes * (size_t)n_images, c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    c->n_images = n_images;
    c->pyr_first = 0;
    c->pyr_count = n_images;
    c->n_frames = n_frames;
    c->w = w;
    c->h = h;
    c->max_pts_set = 0;
    std::fill(c->h_npts.begin(), c->h_npts.end(), 0);
    std::fill(c->h_ntracked.begin(), c->h_ntracked.end(), 0);
    std::fill(c->img_stale.begin(), c->img_stale.end(), 0);
    std::fill(c->h_quads.begin(), c->h_quads.end(), Quad{0, 0, 0, 0});
    c->quads_set = false;
    VO_HIP_TRY(c, hipMemsetAsync(c->d_quads, 0, sizeof(Quad) * c->max_frames, c->sel->stream));
    VO_HIP_TRY(c, hipMemsetAsync(c->d_overflow, 0, sizeof(int) * c->max_frames, c->sel->stream));
    c->detect_uploaded = false; // the per-frame detect flags on the device belong to the previous batch shape
    VO_HIP_TRY(c, hipMemsetAsync(c->d_npts, 0, sizeof(int) * c->max_frames, c->sel->stream));
    c->pts_sel = -1;
    VO_HIP_TRY(c, hipMemsetAsync(c->d_ntracked, 0, sizeof(int) * c->max_frames, c->sel->stream));
    VO_HIP_TRY(c, hipMemsetAsync(c->d_fages, 0, sizeof(int) * (size_t)c->max_frames * c->fcap, c->sel->stream));
    return VO_OK;
}

} // extern "C"

namespace vo_capi {

// A host image into the next page-locked staging slot, row_bytes of each row, the rows `pitch` bytes apart; the points of an
// idle (synchronous) call into their own staging buffer beside it.  Returns the slot.
// zero_gap: the pitch - row_bytes bytes behind every row are zeroed (a raw plane's frame, which the contiguous copy runs over).
static int stage_image(vo_ctx *c, const void *src, int stride, size_t pitch, size_t row_bytes, bool idle, const float *pts, int n_pts,
                       uint8_t **slot, bool zero_gap = false)
{
    if (c->stage_next == 0 && !idle) // all slots may still be in flight from the previous round of uploads
        VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    *slot = c->h_stage + c->stage_slot * (size_t)c->stage_next;
    c->stage_next = (c->stage_next + 1) % VO_STAGE_SLOTS;
    for (int y = 0; y < c->h; y++)
        memcpy(*slot + (size_t)y * pitch, (const uint8_t *)src + (size_t)y * stride, row_bytes);
    for (int y = 0; zero_gap && y < c->h; y++)
        memset(*slot + (size_t)y * pitch + row_bytes, 0, pitch - row_bytes);
    if (idle && n_pts > 0)
        memcpy(c->h_pts_stage, pts, sizeof(float2) * (size_t)n_pts);
    return VO_OK;
}

// upload_image of a context with maps (arguments checked there): the kernels and copies of the plain upload, aimed at raw plane
// idx % VO_STAGE_SLOTS -- pitch rect_raw_pitch, interior only -- then rectify_kernel on the same stream into level 0 of image idx
// with the maps of side idx & 1.  The call's points and count ride with the pull as they always did.
static int upload_image_rectified(vo_ctx *c, int idx, const void *src, int stride, hipMemcpyKind kind, bool idle, const float *pts, int n_pts,
                                  hipStream_t on)
{
    const int fmt = c->prm.input_format, rp = rect_raw_pitch(c->w);
    uint8_t *raw = c->d_rect_raw + (size_t)(idx % VO_STAGE_SLOTS) * c->rect_plane + rect_raw_origin(c->w);
    const bool host = kind == hipMemcpyHostToDevice;
    hipStream_t st = host && idle && on ? on : c->sel->stream;
    c->img_stale[idx] = 1;
    if (fmt != VO_FMT_GRAY8) {
        const void *from = src;
        int from_stride = stride;
        const bool with_pts = host && idle && n_pts >= 0;
        if (host) {
            const size_t rb = fmt_row_bytes(fmt, c->w);
            uint8_t *slot = nullptr;
            int rc = stage_image(c, src, stride, rb, rb, idle, pts, n_pts, &slot);
            if (rc != VO_OK)
                return rc;
            from = c->d_stage + (slot - c->h_stage);
            from_stride = (int)rb;
        }
        if (launch_pull_image_fmt(fmt, from, from_stride, raw, rp, c->w, c->h, st, with_pts ? c->d_pts_stage : nullptr,
                                  with_pts ? c->d_pts : nullptr, with_pts ? n_pts : 0, with_pts ? c->d_npts : nullptr) != 0)
            return fail(c, VO_ERR_STATE, "no converting kernel for this input format");
    } else if (host) {
        // rows at the raw plane's pitch with ZEROS between them: the contiguous copy runs over the frame columns between two rows
        // (and the pull's 16-byte round-up over those behind the last row), which must stay zero
        uint8_t *slot = nullptr;
        int rc = stage_image(c, src, stride, (size_t)rp, (size_t)c->w, idle, pts, n_pts, &slot, /*zero_gap*/ true);
        if (rc != VO_OK)
            return rc;
        const size_t bytes = (size_t)rp * (size_t)(c->h - 1) + (size_t)c->w;
        if (idle)
            launch_pull_image(c->d_stage + (slot - c->h_stage), raw, bytes, st, n_pts >= 0 ? c->d_pts_stage : nullptr, n_pts >= 0 ? c->d_pts : nullptr,
                              n_pts >= 0 ? n_pts : 0, n_pts >= 0 ? c->d_npts : nullptr);
        else
            VO_HIP_TRY(c, hipMemcpyAsync(raw, slot, bytes, hipMemcpyHostToDevice, st));
    } else {
        VO_HIP_TRY(c, hipMemcpy2DAsync(raw, (size_t)rp, src, (size_t)stride, (size_t)c->w, (size_t)c->h, kind, st));
    }
    launch_rectify(c->d_rect_tab + idx, 1, c->w, c->h, rp, c->d_rect_maps, c->lstride[0], c->d_pix + c->loff[0] + (size_t)VO_BY * c->lstride[0] + VO_BX,
                   c->img_bytes, st);
    VO_HIP_TRY(c, hipGetLastError());
    return VO_OK;
}

// vo_set_params with NEW rectification fields, first half: validate, and pack the caller's maps (vo_rectify.h) -- they are read
// here and never again.  Changes nothing of the context.
int rect_check_pack(vo_ctx *c, const vo_params *p, std::vector<uint32_t> *out)
{
    std::vector<uint32_t> &packed = *out;
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "vo_set_params: the rectification maps cannot change inside the lock-step loop");
    if (p->rectify != 0 && p->rectify != 1)
        return fail(c, VO_ERR_ARG, "vo_set_params: rectify is 0 or 1");
    const int w = p->rect_w, h = p->rect_h;
    if (p->rectify) {
        if (w < 32 || h < 32 || w > c->max_w || h > c->max_h)
            return fail(c, VO_ERR_ARG, "vo_set_params: rect_w x rect_h outside 32 x 32 .. the size given to vo_create");
        if (!p->rect_map_x_left || !p->rect_map_y_left || !p->rect_map_x_right || !p->rect_map_y_right)
            return fail(c, VO_ERR_ARG, "vo_set_params: rectify = 1 needs the four maps (rect_map_x / y _left / _right)");
        if (p->rect_map_stride < 4 * w || p->rect_map_stride % 4 != 0)
            return fail(c, VO_ERR_ARG, "vo_set_params: rect_map_stride is in bytes, a multiple of 4 and at least 4 * rect_w");
        packed.resize((size_t)2 * w * h);
        const float *mx[2] = {p->rect_map_x_left, p->rect_map_x_right}, *my[2] = {p->rect_map_y_left, p->rect_map_y_right};
        const size_t ms = (size_t)p->rect_map_stride / 4;
        for (int side = 0; side < 2; side++)
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++)
                    if (!rect_pack(mx[side][y * ms + x], my[side][y * ms + x], x, y, w, h, &packed[((size_t)side * h + y) * w + x]))
                        return fail(c, VO_ERR_ARG, "vo_set_params: a rectification map entry is more than 1023 pixels away from its own "
                                                   "pixel and not wholly outside the image");
    }
    return VO_OK;
}

// ... second half, behind everything else of vo_set_params that can refuse: the old maps, raw planes and table go, the new ones
// are allocated (planes zeroed once), uploaded and written.  A HIP failure here leaves a context WITHOUT maps (rectify = 0).
int rect_commit(vo_ctx *c, const vo_params *p, const std::vector<uint32_t> &packed)
{
    const int w = p->rect_w, h = p->rect_h;
    VO_HIP_TRY(c, hipSetDevice(c->device));
    int rc = sync_all(c); // a queued rectify_kernel may still read the old maps and planes
    if (rc != VO_OK)
        return rc;
    VO_HIP_TRY(c, c->own.give_back(&c->d_rect_maps));
    VO_HIP_TRY(c, c->own.give_back(&c->d_rect_raw));
    VO_HIP_TRY(c, c->own.give_back(&c->d_rect_tab));
    c->rect_plane = 0;
    c->prm.rectify = 0; // (until the new ones are in place)
    if (!p->rectify)
        return VO_OK;
    c->rect_plane = (rect_raw_bytes(w, h) + 255) / 256 * 256;
    std::vector<RectImage> tab((size_t)c->max_images);
    bool ok = c->own.device(&c->d_rect_maps, packed.size());
    ok = ok && c->own.device(&c->d_rect_raw, c->rect_plane * VO_STAGE_SLOTS, /*zero*/ true);
    ok = ok && c->own.device(&c->d_rect_tab, tab.size());
    for (size_t i = 0; ok && i < tab.size(); i++)
        tab[i] = RectImage{c->d_rect_raw + (i % VO_STAGE_SLOTS) * c->rect_plane + rect_raw_origin(w), (int)i, (int)(i & 1)};
    if (ok)
        ok = (c->own.err = hipMemcpy(c->d_rect_maps, packed.data(), sizeof(uint32_t) * packed.size(), hipMemcpyHostToDevice)) == hipSuccess &&
             (c->own.err = hipMemcpy(c->d_rect_tab, tab.data(), sizeof(RectImage) * tab.size(), hipMemcpyHostToDevice)) == hipSuccess;
    if (!ok) {
        const hipError_t e = c->own.err;
        (void)c->own.give_back(&c->d_rect_maps);
        (void)c->own.give_back(&c->d_rect_raw);
        (void)c->own.give_back(&c->d_rect_tab);
        c->n_images = 0; // (the old maps are gone: the context is a plain one until maps are set again)
        return fail_hip(c, "vo_set_params: device memory for the rectification maps and raw planes", e);
    }
    return VO_OK;
}

int upload_image(vo_ctx *c, int idx, const void *src, int stride, hipMemcpyKind kind, bool idle, const float *pts, int n_pts,
                 hipStream_t on, bool plain)
{
    if (!c)
        return VO_ERR_ARG;
    if (c->n_images == 0)
        return fail(c, VO_ERR_STATE, "upload before vo_batch_configure");
    const int fmt = c->prm.input_format;
    if (idx < 0 || idx >= c->n_images || !src || stride < c->w * ingest_bpp(fmt))
        return fail(c, VO_ERR_ARG, "vo_batch_upload_image: bad index / stride (at least w * bytes per pixel of vo_params.input_format)");
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "vo_batch_upload_image inside the sequence loop: use vo_seq_push_pair");
    VO_HIP_TRY(c, hipSetDevice(c->device));
    uint8_t *dst = c->d_pix + (size_t)idx * c->img_bytes + c->loff[0] + (size_t)VO_BY * c->lstride[0] + VO_BX;
    if (c->prm.rectify && !plain)
        return upload_image_rectified(c, idx, src, stride, kind, idle, pts, n_pts, on);
    // the pyramid levels, borders and Scharr images of this image now belong to the previous pixels: LK / DETECT
    // refuse to read it until VO_STAGE_PYRAMID has covered it again (the contiguous host copy below also
    // overwrites the level-0 border columns with staging bytes)
    c->img_stale[idx] = 1;
    if (fmt != VO_FMT_GRAY8) {
        // any other format: the RAW rows go into the page-locked slot (tight, fmt_row_bytes each) and the converting pull kernel
        // (ingest_fmt.hip) writes the gray rows at the device pitch -- for the synchronous calls and the batch upload alike; a
        // device source is converted where it lies
        const void *from = src;
        int from_stride = stride;
        const bool with_pts = kind == hipMemcpyHostToDevice && idle && n_pts >= 0;
        if (kind == hipMemcpyHostToDevice) {
            const size_t rb = fmt_row_bytes(fmt, c->w);
            uint8_t *slot = nullptr;
            int rc = stage_image(c, src, stride, rb, rb, idle, pts, n_pts, &slot);
            if (rc != VO_OK)
                return rc;
            from = c->d_stage + (slot - c->h_stage);
            from_stride = (int)rb;
        }
        hipStream_t st = idle && on ? on : c->sel->stream;
        if (launch_pull_image_fmt(fmt, from, from_stride, dst, c->lstride[0], c->w, c->h, st, with_pts ? c->d_pts_stage : nullptr,
                                  with_pts ? c->d_pts : nullptr, with_pts ? n_pts : 0, with_pts ? c->d_npts : nullptr) != 0)
            return fail(c, VO_ERR_STATE, "no converting kernel for this input format");
        VO_HIP_TRY(c, hipGetLastError());
        return VO_OK;
    }
    if (kind == hipMemcpyHostToDevice) {
        // repack to the device pitch in pinned memory, then one contiguous copy from pixel (0, 0) to the
        // last interior pixel.  The bytes between two rows land in border columns, which the pyramid
        // stage's border fill rewrites before anything reads them.
        const size_t pitch = (size_t)c->lstride[0];
        uint8_t *slot = nullptr;
        int rc = stage_image(c, src, stride, pitch, (size_t)c->w, idle, pts, n_pts, &slot);
        if (rc != VO_OK)
            return rc;
        const size_t bytes = pitch * (size_t)(c->h - 1) + (size_t)c->w;
        if (idle) { // a synchronous drop-in call: the GPU pulls the slot itself (pyramid.hip, launch_pull_image; the 16-byte
                    // round-up of the last row stays inside the row's pitch)
            if (n_pts >= 0) // the call's points (frame 0) and their count with this image
                launch_pull_image(c->d_stage + (slot - c->h_stage), dst, bytes, on ? on : c->sel->stream, c->d_pts_stage, c->d_pts, n_pts, c->d_npts);
            else
                launch_pull_image(c->d_stage + (slot - c->h_stage), dst, bytes, on ? on : c->sel->stream);
            VO_HIP_TRY(c, hipGetLastError());
        } else {
            VO_HIP_TRY(c, hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, c->sel->stream));
        }
        return VO_OK;
    }
    VO_HIP_TRY(c, hipMemcpy2DAsync(dst, (size_t)c->lstride[0], src, (size_t)stride, (size_t)c->w, (size_t)c->h,
                                   kind, c->sel->stream));
    return VO_OK;
}

} // namespace vo_capi

extern "C" {

int vo_batch_upload_image(vo_ctx *c, int idx, const uint8_t *host, int stride)
{
    if (c)
        c->tf_base = -1; // the caller owns the image table now (see vo_ctx::tf_base)
    int rc = upload_image(c, idx, host, stride, hipMemcpyHostToDevice);
    if (rc == VO_OK) // pageable host memory: make the call safe to return from
        VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    return rc;
}

int vo_batch_upload_image_dev(vo_ctx *c, int idx, const void *dev, int stride)
{
    if (c)
        c->tf_base = -1;
    return upload_image(c, idx, dev, stride, hipMemcpyDeviceToDevice);
}

int vo_batch_set_quads(vo_ctx *c, const int32_t *quads4, int n_frames)
{
    if (!c || !quads4)
        return VO_ERR_ARG;
    if (c->n_images == 0 || n_frames != c->n_frames)
        return fail(c, VO_ERR_STATE, "vo_batch_set_quads: configure first / frame count mismatch");
    for (int i = 0; i < 4 * n_frames; i++)
        if (quads4[i] < 0 || quads4[i] >= c->n_images)
            return fail(c, VO_ERR_ARG, "vo_batch_set_quads: image index out of range");
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "vo_batch_set_quads inside the sequence loop");
    if (c->quads_set && memcmp(c->h_quads.data(), quads4, sizeof(Quad) * n_frames) == 0)
        return VO_OK; // the table on the device already says so (the single-frame calls set {0, 1, 2, 3} every time)
    VO_HIP_TRY(c, hipSetDevice(c->device));
    VO_HIP_TRY(c, hipMemcpyAsync(c->d_quads, quads4, sizeof(Quad) * n_frames, hipMemcpyHostToDevice, c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    memcpy(c->h_quads.data(), quads4, sizeof(Quad) * n_frames);
    c->quads_set = true;
    c->quads_cur = c->d_quads; // (a synchronous drop-in call may have left it at one of its constant quadruples)
    return VO_OK;
}

int vo_batch_set_pyramid_range(vo_ctx *c, int first_image, int n_images)
{
    if (!c)
        return VO_ERR_ARG;
    if (c->n_images == 0)
        return fail(c, VO_ERR_STATE, "vo_batch_set_pyramid_range before vo_batch_configure");
    if (first_image < 0 || n_images < 0 || first_image + n_images > c->n_images)
        return fail(c, VO_ERR_ARG, "vo_batch_set_pyramid_range: range outside the image table");
    c->pyr_first = first_image;
    c->pyr_count = n_images;
    return VO_OK;
}

int vo_batch_set_points(vo_ctx *c, int frame, const float *pts, int n)
{
    if (!c)
        return VO_ERR_ARG;
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "vo_batch_set_points inside the sequence loop (vo_seq_* owns the feature state)");
    if (frame < 0 || frame >= c->n_frames || n < 0 || n > c->cap || (n > 0 && !pts))
        return fail(c, VO_ERR_ARG, "vo_batch_set_points: bad frame / more points than max_pts");
    int rcs = sync_all(c); // a queued filter of the previous run still reads the points
    if (rcs != VO_OK)
        return rcs;
    if (c->pts_sel >= 0) { // the other frames keep what the last DETECT stage gave them
        const size_t B = (size_t)c->max_frames, cap = (size_t)c->cap;
        VO_HIP_TRY(c, hipMemcpyAsync(c->d_pts, cur_pts(c), sizeof(float2) * B * cap, hipMemcpyDeviceToDevice, c->sel->stream));
        VO_HIP_TRY(c, hipMemcpyAsync(c->d_ages, cur_ages(c), sizeof(int) * B * cap, hipMemcpyDeviceToDevice, c->sel->stream));
        VO_HIP_TRY(c, hipMemcpyAsync(c->d_npts, cur_npts(c), sizeof(int) * B, hipMemcpyDeviceToDevice, c->sel->stream));
        VO_HIP_TRY(c, hipMemcpyAsync(c->h_npts.data(), c->d_npts, sizeof(int) * c->n_frames, hipMemcpyDeviceToHost,
                                     c->sel->stream));
        VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
        c->pts_sel = -1;
    }
    if (n > 0)
        VO_HIP_TRY(c, hipMemcpyAsync(c->d_pts + (size_t)frame * c->cap, pts, sizeof(float2) * n,
                                     hipMemcpyHostToDevice, c->sel->stream));
    c->h_npts[frame] = n;
    c->pts_on_device = false;
    VO_HIP_TRY(c, hipMemcpyAsync(c->d_npts + frame, &c->h_npts[frame], sizeof(int), hipMemcpyHostToDevice,
                                 c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    c->max_pts_set = 0;
    for (int f = 0; f < c->n_frames; f++)
        c->max_pts_set = c->h_npts[f] > c->max_pts_set ? c->h_npts[f] : c->max_pts_set;
    return VO_OK;
}

int vo_batch_set_features(vo_ctx *c, int frame, const float *pts, int n_pts, const int32_t *ages, int n_ages)
{
    if (!c)
        return VO_ERR_ARG;
    if (c->n_images == 0)
        return fail(c, VO_ERR_STATE, "vo_batch_set_features before vo_batch_configure");
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "vo_batch_set_features inside the sequence loop (vo_seq_* owns the feature state)");
    if (frame < 0 || frame >= c->n_frames || n_pts < 0 || n_ages < n_pts || n_ages > c->fcap ||
        (n_pts > 0 && !pts) || (n_ages > 0 && !ages))
        return fail(c, VO_ERR_ARG, "vo_batch_set_features: bad frame / counts (need n_pts <= n_ages <= capacity)");
    int rcs = sync_all(c);
    if (rcs != VO_OK)
        return rcs;
    // ages beyond n_ages must read as 0 (age of a freshly appended corner, feature.cpp:260)
    VO_HIP_TRY(c, hipMemsetAsync(c->d_fages + (size_t)frame * c->fcap, 0, sizeof(int) * (size_t)c->fcap, c->sel->stream));
    if (n_pts > 0)
        VO_HIP_TRY(c, hipMemcpyAsync(c->d_feat + (size_t)frame * c->fcap, pts, sizeof(float2) * n_pts,
                                     hipMemcpyHostToDevice, c->sel->stream));
    if (n_ages > 0)
        VO_HIP_TRY(c, hipMemcpyAsync(c->d_fages + (size_t)frame * c->fcap, ages, sizeof(int) * n_ages,
                                     hipMemcpyHostToDevice, c->sel->stream));
    c->h_ntracked[frame] = n_pts;
    VO_HIP_TRY(c, hipMemcpyAsync(c->d_ntracked + frame, &c->h_ntracked[frame], sizeof(int), hipMemcpyHostToDevice,
                                 c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    return VO_OK;
}

int vo_batch_set_detect_params(vo_ctx *c, const vo_detect_params *dp)
{
    if (!c)
        return VO_ERR_ARG;
    if (!dp) {
        vo_default_detect_params(&c->dprm);
        return VO_OK;
    }
    if (dp->features_per_bucket < 1 || dp->features_per_bucket > 8 || dp->bucket_size < 0)
        return fail(c, VO_ERR_ARG, "vo_batch_set_detect_params: features_per_bucket must be 1..8, bucket_size >= 0");
    c->dprm = *dp;
    return VO_OK;
}

int vo_batch_get_features(vo_ctx *c, int frame, float *pts, int32_t *ages, int *n)
{
    if (!c || !n)
        return VO_ERR_ARG;
    if (frame < 0 || frame >= c->n_frames)
        return fail(c, VO_ERR_ARG, "vo_batch_get_features: bad frame");
    VO_HIP_TRY(c, hipSetDevice(c->device));
    int k = 0;
    VO_HIP_TRY(c, hipMemcpyAsync(&k, cur_npts(c) + frame, sizeof(int), hipMemcpyDeviceToHost, c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    if (pts && k > 0)
        VO_HIP_TRY(c, hipMemcpyAsync(pts, cur_pts(c) + (size_t)frame * c->cap, sizeof(float2) * k, hipMemcpyDeviceToHost,
                                     c->sel->stream));
    if (ages && k > 0)
        VO_HIP_TRY(c, hipMemcpyAsync(ages, cur_ages(c) + (size_t)frame * c->cap, sizeof(int) * k, hipMemcpyDeviceToHost,
                                     c->sel->stream));
    int ovf = 0;
    VO_HIP_TRY(c, hipMemcpyAsync(&ovf, c->d_overflow + frame, sizeof(int), hipMemcpyDeviceToHost, c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    *n = k;
    return ovf ? fail_overflow(c, ovf) : VO_OK;
}

int vo_batch_set_projection(vo_ctx *c, const float *P_l, const float *P_r)
{
    if (!c || !P_l || !P_r)
        return VO_ERR_ARG;
    if (c->have_P && memcmp(c->h_P, P_l, 12 * sizeof(float)) == 0 && memcmp(c->h_P + 12, P_r, 12 * sizeof(float)) == 0)
        return VO_OK; // unchanged since the last call (every vo_track_frame passes the same calibration)
    memcpy(c->h_P, P_l, 12 * sizeof(float));
    memcpy(c->h_P + 12, P_r, 12 * sizeof(float));
    VO_HIP_TRY(c, hipSetDevice(c->device));
    VO_HIP_TRY(c, hipMemcpyAsync(c->d_P, c->h_P, 24 * sizeof(float), hipMemcpyHostToDevice, c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    c->have_P = true;
    return VO_OK;
}

} // extern "C"

namespace vo_capi {

// working set of the essential-matrix chain, allocated the first time it is asked for
int ensure_em(vo_ctx *c)
{
    if (c->em_ready)
        return VO_OK;
    VO_HIP_TRY(c, hipSetDevice(c->device));
    const size_t B = (size_t)c->max_frames, cap = (size_t)c->cap;
    Owner &o = c->own;
    bool ok = o.device(&c->em.q0, B * cap) && o.device(&c->em.q1, B * cap) && o.device(&c->em.subsets, B * EM_MAX_ITERS * 5) &&
              o.device(&c->em.rstate, B) && o.device(&c->em.models, B * 128 * 90) && o.device(&c->em.nmodels, B * 128) &&
              o.device(&c->em.counts, B * 128 * 10) && o.device(&c->em.bestE, B * 9) && o.device(&c->em.mask, B * cap);
    for (auto &b : c->pb)
        ok = ok && o.device(&b.em_results, B, /*zero*/ true);
    if (!ok)
        return fail_hip(c, "working set of the essential-matrix chain", o.err);
    c->em_ready = true;
    return VO_OK;
}

} // namespace vo_capi

extern "C" {

int vo_batch_run(vo_ctx *c, int stages)
{
    if (!c)
        return VO_ERR_ARG;
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "vo_batch_run inside the sequence loop: use vo_seq_step");
    return run_stages_auto(c, stages, false);
}

int vo_batch_run_timed(vo_ctx *c, int stages, float *ms)
{
    if (!c || !ms)
        return VO_ERR_ARG;
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "vo_batch_run_timed inside the sequence loop: use vo_seq_step");
    int rc = run_stages_auto(c, stages, true);
    if (rc != VO_OK)
        return rc;
    rc = sync_all(c);
    if (rc != VO_OK)
        return rc;
    for (int s = 0; s < VO_NUM_STAGES; s++) // PYRAMID, DETECT, LK on the tracking stream; the rest on the post stream
        VO_HIP_TRY(c, hipEventElapsedTime(&ms[s], c->ev[stage_events(s).start], c->ev[stage_events(s).end]));
    return VO_OK;
}

int vo_batch_run_slot(vo_ctx *c, int stages, int slot)
{
    if (!c || slot < 0 || slot >= VO_EVENT_SLOTS)
        return VO_ERR_ARG;
    if (c->seq.on)
        return fail(c, VO_ERR_STATE, "vo_batch_run_slot inside the sequence loop: use vo_seq_step");
    return run_stages_auto(c, stages, true, &c->ring[(size_t)slot * (VO_EV_PER_RUN)]);
}

int vo_batch_slot_times(vo_ctx *c, int slot, float *ms)
{
    if (!c || !ms || slot < 0 || slot >= VO_EVENT_SLOTS)
        return VO_ERR_ARG;
    VO_HIP_TRY(c, hipSetDevice(c->device));
    hipEvent_t *evs = &c->ring[(size_t)slot * (VO_EV_PER_RUN)];
    for (int s = 0; s < VO_NUM_STAGES; s++)
        VO_HIP_TRY(c, hipEventElapsedTime(&ms[s], evs[stage_events(s).start], evs[stage_events(s).end]));
    return VO_OK;
}

int vo_batch_sync(vo_ctx *c)
{
    if (!c)
        return VO_ERR_ARG;
    return sync_all(c);
}

int vo_batch_get_tracks(vo_ctx *c, int frame, float *r0, float *r1, float *l1, float *l0_ret, uint8_t *status4,
                        int n)
{
    if (!c)
        return VO_ERR_ARG;
    if (frame < 0 || frame >= c->n_frames || n < 0 || n > c->cap)
        return fail(c, VO_ERR_ARG, "vo_batch_get_tracks: bad frame / n");
    VO_HIP_TRY(c, hipSetDevice(c->device));
    const size_t cap = c->cap;
    const float2 *t = c->d_trk2[c->trk_last] + (size_t)frame * 4 * cap;
    D2H(r0, t, sizeof(float2) * n);
    D2H(r1, t + cap, sizeof(float2) * n);
    D2H(l1, t + 2 * cap, sizeof(float2) * n);
    D2H(l0_ret, t + 3 * cap, sizeof(float2) * n);
    if (status4)
        for (int hop = 0; hop < 4; hop++)
            D2H(status4 + (size_t)hop * n, c->d_status2[c->trk_last] + ((size_t)frame * 4 + hop) * cap, (size_t)n);
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    return VO_OK;
}

int vo_batch_get_filtered(vo_ctx *c, int frame, float *l0, float *r0, float *l1, float *r1, float *xyz,
                          int32_t *keep_idx, int *n_out, int32_t *keep_idx_circ, int *n_circ)
{
    if (!c)
        return VO_ERR_ARG;
    if (frame < 0 || frame >= c->n_frames)
        return fail(c, VO_ERR_ARG, "vo_batch_get_filtered: bad frame");
    int rcs = sync_all(c);
    if (rcs != VO_OK)
        return rcs;
    const vo_ctx::PoseBufs &pb = c->pb[c->last];
    int nAB[2] = {0, 0};
    VO_HIP_TRY(c, hipMemcpyAsync(&nAB[0], c->d_nA + frame, sizeof(int), hipMemcpyDeviceToHost, c->sel->stream));
    VO_HIP_TRY(c, hipMemcpyAsync(&nAB[1], pb.nB + frame, sizeof(int), hipMemcpyDeviceToHost, c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    const size_t cap = c->cap;
    const int K = nAB[1], M = nAB[0];
    const float2 *b = pb.outB + (size_t)frame * 4 * cap;
    D2H(l0, b, sizeof(float2) * K);
    D2H(r0, b + cap, sizeof(float2) * K);
    D2H(l1, b + 2 * cap, sizeof(float2) * K);
    D2H(r1, b + 3 * cap, sizeof(float2) * K);
    D2H(xyz, pb.xyz + (size_t)frame * cap * 3, sizeof(float) * 3 * K);
    D2H(keep_idx, pb.idxB + (size_t)frame * cap, sizeof(int32_t) * K);
    D2H(keep_idx_circ, c->d_idxA + (size_t)frame * cap, sizeof(int32_t) * M);
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    if (n_out)
        *n_out = K;
    if (n_circ)
        *n_circ = M;
    return VO_OK;
}

} // extern "C"

namespace vo_capi {

// PnpParams of the context; K: the caller's intrinsic matrix, else projMatrl(0:3, 0:3) (visualOdometry.cpp:163-165)
PnpParams pnp_params(const vo_ctx *c, const float *K)
{
    PnpParams pp;
    pp.iters = c->prm.ransac_iterations;
    pp.reproj = c->prm.ransac_reproj_error;
    pp.confidence = c->prm.ransac_confidence;
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++)
            pp.K[r * 3 + k] = K ? K[r * 3 + k] : c->h_P[r * 4 + k];
    return pp;
}

LkParams lk_params(const vo_ctx *c)
{
    LkParams lp;
    lp.max_level = c->levels - 1;
    int mc = c->prm.lk_max_count;
    lp.max_count = mc < 0 ? 0 : mc > 100 ? 100 : mc;
    double eps = c->prm.lk_epsilon;
    eps = eps < 0. ? 0. : eps > 10. ? 10. : eps;
    lp.epsilon = eps * eps;
    lp.min_eig = (float)c->prm.lk_min_eig_threshold;
    lp.full_chain = c->prm.lk_full_chain;
    return lp;
}

// findEssentialMat's arguments in a run with vo_params.mono_rotation: focal length and principal point of projMatrl with the
// context's em_prob / em_threshold (vo_essential_pose passes its caller's five instead)
EmParams em_params(const vo_ctx *c)
{
    return EmParams{(double)c->h_P[0], (double)c->h_P[2], (double)c->h_P[6], c->prm.em_prob, c->prm.em_threshold, EM_MAX_ITERS};
}

// the context holds the t1 pair of a previous synchronous call of this size, pyramids built (vo_ctx::tf_base; stale: the call
// that uploaded the pair failed before its pyramids were built)
bool have_kept_pair(const vo_ctx *c, int w, int h)
{
    return c->tf_base >= 0 && !c->seq.on && c->n_images == 4 && c->n_frames == 1 && c->w == w && c->h == h && !c->img_stale[c->tf_base] &&
           !c->img_stale[c->tf_base + 1];
}

int fail_overflow(vo_ctx *c, int ovf) // ovf: a frame's VO_STAGE_DETECT capacity flags (vo_ctx::d_overflow)
{
    return fail(c, VO_ERR_OVERFLOW, ovf & 1 ? "VO_STAGE_DETECT: carried + detected features exceed the feature-list "
                                              "capacity (4 x max_pts, >= 16384, >= w * h / 16): bucketed set truncated"
                                            : "VO_STAGE_DETECT: the bucketed set exceeds max_pts");
}

int fail_too_few_pnp(vo_ctx *c)
{
    return fail(c, VO_ERR_TOO_FEW, "fewer than 4 correspondences reached solvePnPRansac (CV_Assert(npoints >= 4))");
}

// THE rule by which a frame's pose reaches the caller's rvec / tvec / R (every pointer optional).  r: the PnP side; e: the
// essential-matrix side under mono_rotation, else null.  pnp_rotation: R = Rodrigues(rvec) even under mono_rotation
// (vo_pnp_ransac).  Returns the status of the essential-matrix side (1 ok, 0 no model, -1 too few points), 1 without one.
int deliver_pose(const vo_ctx *c, const PnpResult &r, const EmResult *e, double *rvec, double *tvec, double *R, bool pnp_rotation, bool io_pose)
{
    const bool R_from_pnp = pnp_rotation || !c->prm.mono_rotation; // `if (!mono_rotation) Rodrigues(rvec, rotation)` (visualOdometry.cpp:186-189)
    if (r.status == 0 && r.lm_iters < 0 && io_pose) {
        // four points, P3P without a solution: solvePnP returned false and never wrote rvec / tvec -- the caller's
        // buffers stay as they are; the reference then still runs Rodrigues(rvec, rotation) on what rvec holds.
        // (io_pose = false, vo_batch_get_pose: its rvec / tvec / R are pure OUTPUTS -- a batch frame has no caller pose -- and
        // receive what the kernel left: rvec = 0 like the reference's `cv::Mat::zeros` at visualOdometry.cpp:162, tvec = 0,
        // R = identity, never a Rodrigues of uninitialised memory)
        if (R && rvec && R_from_pnp)
            rodrigues_v2m(rvec, R, nullptr);
    } else if (r.status >= 0) {
        if (rvec)
            memcpy(rvec, r.rvec, sizeof(r.rvec));
        if (tvec)
            memcpy(tvec, r.tvec, sizeof(r.tvec));
        if (R && R_from_pnp)
            memcpy(R, r.R, sizeof(r.R));
    }
    if (!e)
        return 1;
    if (e->status == 1 && R) // rotation = recoverPose's; left untouched when no essential matrix was found (OpenCV throws there)
        memcpy(R, e->R, sizeof(e->R));
    return e->status;
}

// em_status (optional): status of the essential-matrix side of the frame under mono_rotation, 1 otherwise.
int get_pose_impl(vo_ctx *c, int frame, double *rvec, double *tvec, double *R, int32_t *inliers,
                         int *n_inliers, int *status, int32_t *dbg4, bool pnp_rotation, int *em_status, bool io_pose)
{
    if (!c)
        return VO_ERR_ARG;
    if (frame < 0 || frame >= c->n_frames)
        return fail(c, VO_ERR_ARG, "vo_batch_get_pose: bad frame");
    int rcs = sync_all(c);
    if (rcs != VO_OK)
        return rcs;
    const vo_ctx::PoseBufs &pb = c->pb[c->last];
    PnpResult r;
    VO_HIP_TRY(c, hipMemcpyAsync(&r, pb.results + frame, sizeof(r), hipMemcpyDeviceToHost, c->sel->stream));
    VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    EmResult e;
    const bool mono = !pnp_rotation && c->prm.mono_rotation && c->em_ready;
    if (mono)
        VO_HIP_TRY(c, hipMemcpy(&e, pb.em_results + frame, sizeof(e), hipMemcpyDeviceToHost));
    const int ems = deliver_pose(c, r, mono ? &e : nullptr, rvec, tvec, R, pnp_rotation, io_pose);
    if (em_status)
        *em_status = ems;
    if (inliers && r.n_inliers > 0) {
        D2H(inliers, pb.inliers + (size_t)frame * c->cap, sizeof(int32_t) * r.n_inliers);
        VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    }
    if (n_inliers)
        *n_inliers = r.n_inliers;
    if (status)
        *status = r.status;
    if (dbg4) {
        dbg4[0] = r.niters;
        dbg4[1] = r.best_iter;
        dbg4[2] = r.max_good;
        dbg4[3] = r.lm_iters;
    }
    return VO_OK;
}

} // namespace vo_capi

extern "C" {

int vo_batch_get_pose(vo_ctx *c, int frame, double *rvec, double *tvec, double *R, int32_t *inliers,
                      int *n_inliers, int *status, int32_t *dbg4)
{
    return get_pose_impl(c, frame, rvec, tvec, R, inliers, n_inliers, status, dbg4, false, nullptr, /*io_pose*/ false);
}

int vo_batch_get_essential(vo_ctx *c, int frame, double *E, double *R, double *t, uint8_t *mask, int n,
                           int *n_inliers, int *n_good, int *status, int32_t *dbg2)
{
    if (!c)
        return VO_ERR_ARG;
    if (frame < 0 || frame >= c->n_frames || n < 0 || n > c->cap)
        return fail(c, VO_ERR_ARG, "vo_batch_get_essential: bad frame / n");
    if (!c->em_ready)
        return fail(c, VO_ERR_STATE, "vo_batch_get_essential: no run with vo_params.mono_rotation yet");
    int rcs = sync_all(c);
    if (rcs != VO_OK)
        return rcs;
    EmResult e;
    VO_HIP_TRY(c, hipMemcpy(&e, c->pb[c->last].em_results + frame, sizeof(e), hipMemcpyDeviceToHost));
    if (e.status == 1) {
        if (E)
            memcpy(E, e.E, sizeof(e.E));
        if (R)
            memcpy(R, e.R, sizeof(e.R));
        if (t)
            memcpy(t, e.t, sizeof(e.t));
        if (mask && n > 0)
            VO_HIP_TRY(c, hipMemcpy(mask, c->em.mask + (size_t)frame * c->cap, (size_t)n, hipMemcpyDeviceToHost));
    }
    if (n_inliers)
        *n_inliers = e.n_inliers;
    if (n_good)
        *n_good = e.n_good;
    if (status)
        *status = e.status;
    if (dbg2) {
        dbg2[0] = e.niters;
        dbg2[1] = e.best;
    }
    return VO_OK;
}

int vo_essential_pose(vo_ctx *c, const float *pts0, const float *pts1, int n, double focal, double ppx, double ppy,
                      double prob, double threshold, double *E, double *R, double *t, uint8_t *mask, int *n_good)
{
    if (!c || n < 0 || (n > 0 && (!pts0 || !pts1)) || !(prob > 0 && prob < 1) || !(threshold > 0) || !(focal != 0))
        return VO_ERR_ARG;
    if (n > c->cap)
        return fail(c, VO_ERR_ARG, "more points than max_pts given to vo_create");
    int rcs = sync_all(c);
    if (rcs != VO_OK)
        return rcs;
    rcs = ensure_em(c);
    if (rcs != VO_OK)
        return rcs;
    vo_ctx::PoseBufs &pb = c->pb[c->last];
    const size_t cap = (size_t)c->cap;
    if (n > 0) {
        VO_HIP_TRY(c, hipMemcpyAsync(pb.outB, pts0, sizeof(float2) * n, hipMemcpyHostToDevice, c->sel->stream));
        VO_HIP_TRY(c, hipMemcpyAsync(pb.outB + 2 * cap, pts1, sizeof(float2) * n, hipMemcpyHostToDevice, c->sel->stream));
    }
    VO_HIP_TRY(c, hipMemcpyAsync(pb.nB, &n, sizeof(int), hipMemcpyHostToDevice, c->sel->stream));
    if (c->n_frames < 1)
        c->n_frames = 1;
    launch_essential(pb.outB, pb.outB + 2 * cap, 4 * cap, pb.nB, c->cap, 1, EmParams{focal, ppx, ppy, prob, threshold, EM_MAX_ITERS}, c->em, pb.em_results,
                     /*crowded*/ standalone_waves(c) >= 2, c->sel->stream);
    VO_HIP_TRY(c, hipGetLastError());
    int status = 0, good = 0;
    int rc = vo_batch_get_essential(c, 0, E, R, t, mask, n, nullptr, &good, &status, nullptr);
    if (rc != VO_OK)
        return rc;
    if (n_good)
        *n_good = good;
    if (status < 0)
        return fail(c, VO_ERR_TOO_FEW, "fewer than 5 correspondences reached findEssentialMat");
    return status == 1 ? VO_OK : 1;
}

int vo_batch_get_pyramid_level(vo_ctx *c, int idx, int level, uint8_t *out, int *w_l, int *h_l)
{
    if (!c)
        return VO_ERR_ARG;
    if (idx < 0 || idx >= c->n_images || level < 0 || level >= c->levels)
        return fail(c, VO_ERR_ARG, "vo_batch_get_pyramid_level: bad image / level");
    VO_HIP_TRY(c, hipSetDevice(c->device));
    if (w_l)
        *w_l = c->lw[level];
    if (h_l)
        *h_l = c->lh[level];
    if (out) {
        VO_HIP_TRY(c, hipMemcpy2DAsync(out, (size_t)c->lw[level],
                                       c->d_pix + (size_t)idx * c->img_bytes + c->loff[level] +
                                           (size_t)VO_BY * c->lstride[level] + VO_BX,
                                       (size_t)c->lstride[level], (size_t)c->lw[level], (size_t)c->lh[level],
                                       hipMemcpyDeviceToHost, c->sel->stream));
        VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    }
    return VO_OK;
}

int vo_batch_get_level_planes(vo_ctx *c, int idx, int level, uint8_t *pix, uint32_t *der, int *stride, int *rows)
{
    if (!c)
        return VO_ERR_ARG;
    if (idx < 0 || idx >= c->n_images || level < 0 || level >= c->levels)
        return fail(c, VO_ERR_ARG, "vo_batch_get_level_planes: bad image / level");
    VO_HIP_TRY(c, hipSetDevice(c->device));
    const int n_rows = c->lh[level] + 2 * VO_BY;
    if (stride)
        *stride = c->lstride[level];
    if (rows)
        *rows = n_rows;
    const size_t off = (size_t)idx * c->img_bytes + c->loff[level], n = (size_t)c->lstride[level] * n_rows;
    if (pix)
        VO_HIP_TRY(c, hipMemcpyAsync(pix, c->d_pix + off, n, hipMemcpyDeviceToHost, c->sel->stream));
    if (der)
        VO_HIP_TRY(c, hipMemcpyAsync(der, c->d_der + off, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->sel->stream));
    if (pix || der)
        VO_HIP_TRY(c, hipStreamSynchronize(c->sel->stream));
    return VO_OK;
}

int vo_model_bytes(const vo_ctx *c, int w, int h, int n_points, double *b)
{
    if (!c || !b || w < 1 || h < 1 || n_points < 0)
        return VO_ERR_ARG;
    // B_pyr = 4 images x (read sum_{l<L} S_l + write sum_{l>=1} S_l)
    int L = c->prm.lk_max_level, cw = w, ch = h;
    double rd = 0, wr = 0;
    int lv = 0;
    for (int l = 0; l <= L; l++) {
        double S = (double)cw * ch;
        if (l < L)
            rd += S;
        if (l >= 1)
            wr += S;
        lv = l;
        int nw = (cw + 1) / 2, nh = (ch + 1) / 2;
        if (nw <= 21 || nh <= 21)
            break;
        cw = nw;
        ch = nh;
    }
    (void)lv;
    b[0] = 4.0 * (rd + wr);
    // B_lk = 4 hops x N x [(L+1) x ((win+3)^2 + (win+1)^2) + 8 + 8 + 1]
    b[1] = 4.0 * n_points * ((L + 1) * (576.0 + 484.0) + 17.0);
    b[2] = 48.0 * n_points + 48.0;
    return VO_OK;
}

} // extern "C"
