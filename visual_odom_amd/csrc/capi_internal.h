// capi_internal.h -- what the translation units of the C ABI share: the context record, the stream set, small helpers and the
// internal functions one unit calls in another.  capi.hip: context, allocation, batch API and getters; capi_run.hip: the stage
// launcher (run_stages); capi_sched.hip: the schedule probe and its export / import; capi_seq.hip: the lock-step sequence
// loop; capi_dropin.hip: the synchronous drop-in calls; capi_detector.hip: the frame loop's detector.  Round 4 split capi.hip (2 800 lines in one unit)
// without changing behaviour.  Nothing declared here is exported: internal functions live in namespace vo_capi.
#pragma once
#include "../../include/vo_fast_mask.h" // (brings vo_topup.h, vo_detector.h, vo_hip.h and the three corner headers)
#include "vo_kernels.h"
#include "vo_dev_hooks.h"
#include "vo_integrate.h"
#include "vo_linalg.h"
#include "vo_rectify.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <vector>

using namespace vo;
namespace vo {
struct CornArgs; // vo_corners_dev.h
}

#define VO_SEQ_INFLIGHT 8 // steps the host may run ahead of the device
// timing events of one run: [0..3] tracking stream (3 stages), [4..7] post streams (3 stages), [8] start of DETECT on
// the tracking stream (differs from [1] when the pyramid stage runs on the lock-step loop's prepare stream)
#define VO_EV_PER_RUN (VO_NUM_STAGES + 3)
#define VO_SEQ_MAX_RING 3

// A cross-stream dependency: an event (handed out by an Owner) and whether it has been recorded and not yet waited for.  Whoever
// writes what the other side reads records; whoever is about to overwrite or read it waits -- once: a signal nobody recorded, or
// that has been waited for already, costs no HIP call.  Forgetting is for after a full drain (seq_forget).
struct Signal {
    hipEvent_t ev = nullptr;
    bool pending = false;
    hipError_t record(hipStream_t s)
    {
        pending = true;
        return hipEventRecord(ev, s);
    }
    hipError_t wait(hipStream_t s) { return take() ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; } // stream s waits, if pending
    hipError_t wait_host() { return take() ? hipEventSynchronize(ev) : hipSuccess; }               // the calling thread waits, if pending
    void forget() { pending = false; }
    bool take() // clears the flag and says whether it was set
    {
        const bool was = pending;
        pending = false;
        return was;
    }
};

// Device memory, page-locked host memory and events of ONE lifetime (a context; a configuration of the lock-step loop): handed
// out here, recorded, and released together.  The typed pointers the kernels and getters use stay where they are -- members of
// vo_ctx -- and own nothing.  A request that fails leaves its pointer null and the HIP error in `err`.
struct Owner {
    std::vector<void *> dev, host;
    std::vector<hipEvent_t> events;
    hipError_t err = hipSuccess;
    template <typename T>
    bool device(T **p, size_t n, bool zero = false) // n elements
    {
        if ((err = hipMalloc((void **)p, n * sizeof(T))) != hipSuccess) {
            *p = nullptr;
            return false;
        }
        dev.push_back(*p);
        return !zero || (err = hipMemset(*p, 0, n * sizeof(T))) == hipSuccess;
    }
    // flags: hipHostMallocMapped / hipHostMallocDefault; alias (optional): the address the GPU reads and writes the memory at
    template <typename T>
    bool pinned(T **p, size_t bytes, unsigned flags, uint8_t **alias = nullptr)
    {
        if ((err = hipHostMalloc((void **)p, bytes, flags)) != hipSuccess) {
            *p = nullptr;
            return false;
        }
        host.push_back(*p);
        return !alias || (err = hipHostGetDevicePointer((void **)alias, *p, 0)) == hipSuccess;
    }
    bool event(hipEvent_t *e, bool timing = false)
    {
        if ((err = timing ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming)) != hipSuccess) {
            *e = nullptr;
            return false;
        }
        events.push_back(*e);
        return true;
    }
    bool signal(Signal *s) { return event(&s->ev); }
    template <typename T>
    hipError_t give_back(T **p) // one buffer (device or host) now: a buffer that is regrown
    {
        void *v = *p;
        *p = nullptr;
        for (std::vector<void *> *list : {&dev, &host})
            for (size_t i = 0; v && i < list->size(); i++)
                if ((*list)[i] == v) {
                    list->erase(list->begin() + i);
                    return list == &dev ? hipFree(v) : hipHostFree(v);
                }
        return hipSuccess;
    }
    void release()
    {
        for (void *p : dev)
            (void)hipFree(p);
        for (void *p : host)
            (void)hipHostFree(p);
        for (hipEvent_t e : events)
            (void)hipEventDestroy(e);
        dev.clear();
        host.clear();
        events.clear();
    }
};

// The HIP streams of one context (pooled per device, see acquire_streams).  One table, twice: the ordinary set and its
// PARTITIONED twin on two disjoint halves of the compute units (capi.hip, ensure_partitioned_streams) -- the one-sequence
// lock-step loop runs on that; vo_ctx::sel points at the one the context enqueues on.
struct Streams {
    hipStream_t stream = nullptr;                                          // tracking stream
    hipStream_t pnp = nullptr, pnp2 = nullptr, filter = nullptr, em = nullptr; // post-LK streams
    hipStream_t copy = nullptr, prep = nullptr; // lock-step loop's ingest: plain copy stream / highest-priority prepare stream
};
// THE list of a set's streams, in the order the partitioned twin creates them.  TRACK and INGEST streams get one half of the
// compute units there and POST streams the other; the INGEST streams of the ordinary set are created on first use.
enum StreamRole { TRACK, POST, INGEST };
struct StreamSlot {
    hipStream_t Streams::*m;
    StreamRole role;
};
static const StreamSlot VO_STREAM_SLOTS[] = {{&Streams::stream, TRACK}, {&Streams::pnp, POST},    {&Streams::pnp2, POST}, {&Streams::filter, POST},
                                            {&Streams::em, POST},      {&Streams::copy, INGEST}, {&Streams::prep, INGEST}};
struct StreamSet {
    Streams plain, part;
    bool part_tried = false;
    int id = 0; // creation rank on its device: the pool hands out the oldest free set first
};

struct vo_ctx {
    int device = 0;
    StreamSet streams;
    Streams *sel = &streams.plain; // the twin every launch goes to (select_streams)
    Owner own;                    // everything allocated for the context's lifetime
    int max_w = 0, max_h = 0, cap = 0, max_frames = 0, max_images = 0;
    vo_params prm;
    hipEvent_t ev[VO_EV_PER_RUN] = {}; // [0..3] tracking stream (3 stages), [4..7] post stream (3 stages)
    std::vector<hipEvent_t> ring; // VO_EVENT_SLOTS x (VO_EV_PER_RUN) for vo_batch_run_slot
    std::string err;

    // batch configuration
    int n_images = 0, n_frames = 0, w = 0, h = 0, levels = 0; // levels = max_level + 1 actually built
    int lw[VO_MAX_LEVELS] = {}, lh[VO_MAX_LEVELS] = {}, lstride[VO_MAX_LEVELS] = {};
    size_t loff[VO_MAX_LEVELS] = {}, img_bytes = 0;
    int pyr_first = 0, pyr_count = 0; // image range VO_STAGE_PYRAMID rebuilds
    int max_pts_set = 0; // largest n over the frames of the batch (or its bound after VO_STAGE_DETECT)
    bool pts_on_device = false, detect_uploaded = false;

    // device memory
    uint8_t *d_pix = nullptr;  // all bordered pyramids, image i at d_pix + i * img_bytes
    uint32_t *d_der = nullptr; // all Scharr pyramids (one dword per pixel), image i at d_der + i * img_bytes
    size_t pix_capacity = 0;   // in pixels (bytes of d_pix, dwords of d_der)
    PyrImage *d_imgs = nullptr;
    Quad *d_quads = nullptr;
    float2 *d_pts = nullptr, *d_outA = nullptr;
    // LK outputs (4 hops of positions + status per frame) are double-buffered: LK of run k + 1 writes one set
    // while the filter of run k still reads the other, so the tracking stream never idles behind the filter
    float2 *d_trk2[2] = {};
    uint8_t *d_status2[2] = {};
    Signal trk_free[2]; // recorded after the filter has read that set (and d_pts)
    int trk_next = 0, trk_last = 0; // set the next LK writes / set the latest LK wrote
    // The bucketed feature set VO_STAGE_DETECT produces belongs to the same set as the tracks made from it, so
    // DETECT of run k + 1 never waits for the filter of run k either.  pts_sel = -1: the current features are
    // the host-set ones (d_pts / d_npts / d_ages, vo_batch_set_points); else the DETECT output of that set.
    float2 *d_pts_det[2] = {};
    int *d_npts_det[2] = {}, *d_ages_det[2] = {};
    int pts_sel = -1;
    int *d_npts = nullptr, *d_nA = nullptr, *d_idxA = nullptr;
    float *d_P = nullptr; // d_P: P_l (12) then P_r (12)
    // Everything the pose solve reads or writes exists twice: the PnP/RANSAC chain of batch k runs on
    // its own stream while the tracking stages of batch k + 1 already fill the other set.
    struct PoseBufs {
        float2 *outB = nullptr;  // [B][4][cap] l0, r0, l1, r1 after the consistency filter
        int *idxB = nullptr, *nB = nullptr;
        float *xyz = nullptr;
        int32_t *subsets = nullptr, *inliers = nullptr;
        double *models = nullptr;
        int *counts = nullptr;
        RansacState *rstate = nullptr;
        PnpResult *results = nullptr;
        EmResult *em_results = nullptr; // mono_rotation branch (allocated with the rest of `em` on first use)
        double *epnp_ws = nullptr;      // workspace of the four-kernel EPnP (small launches, pnp.hip)
        double *rest_ws = nullptr;      // ransac_rest_kernel's 12 x 12 matrices [min(max_frames, VO_EPNP_WS_MAX_FRAMES)][groups][156][64]
        double *epnp_gws = nullptr;     // developer build: the slim chain's 12 x 12 matrices [max_frames][VO_EPNP_GWS_BLOCKS][156][64]
        hipEvent_t ready = nullptr, tri_done = nullptr; // LK done / triangulation done
        hipEvent_t em_done = nullptr; // essential-matrix chain done (mono_rotation)
        Signal done;                  // pose solve done
    } pb[2];
    int cur = 0, last = 0; // set the next run writes / set the last run wrote
    // findEssentialMat + recoverPose working set (vo_params.mono_rotation / vo_essential_pose): one copy, only
    // ever touched on the pose stream, allocated on first use
    EmBufs em;
    bool em_ready = false;
    // detection / bucketing (VO_STAGE_DETECT)
    vo_detect_params dprm;
    int fcap = 0;                  // capacity of the carried + detected feature list of a frame
    unsigned long long *d_nmsmask = nullptr; // [B][max_h][ceil(max_w / 64)] NMS keep ballots
    int *d_rowcnt = nullptr;       // [B][max_h] corners per image row (zero between launches)
    int *d_rowoff = nullptr;       // [B][max_h] exclusive row offsets
    int *d_detect = nullptr, *d_ntracked = nullptr, *d_nnew = nullptr; // [B]
    float2 *d_feat = nullptr;      // [B][fcap] carried features, then the new corners
    int *d_fages = nullptr;        // [B][fcap] ages of d_feat (zero beyond the uploaded ages)
    int *d_ages = nullptr;         // [B][cap] ages of the bucketed set (parallel to d_pts)
    std::vector<int> h_ntracked, h_detect;
    // second pose stream (Streams::pnp2): in a SMALL batch the pose chain is a few latency-bound waves (1.0-1.3 ms for one frame) and
    // longer than the tracking stages of the next run, so back-to-back runs were throttled by it (lock-step loop with
    // one sequence: 1.35 ms per step, of which 1.3 ms waiting behind the previous step's chain).  Runs alternate between
    // the two buffer sets anyway; giving each set its own stream lets two chains overlap.  Whether that pays is part of
    // the SCHEDULE, which is probed, not looked up (see Schedule below).
    // How the pose chain is scheduled next to the tracking stages -- three knobs, none of which changes a result:
    //   waves   register budget of the f64 pose kernels as waves per SIMD: 1 = 512 registers (fastest alone, but such a
    //           wave only starts on a completely empty SIMD and keeps the next run's kernels waiting), 2 = 256 registers
    //   streams 1 or 2 pose streams (2: the chains of consecutive runs overlap)
    //   prep    lock-step loop only: the new pairs' pyramids + FAST of their left images on the prepare stream, one step
    //           ahead and off the tracking stream's critical path
    // Round 2 chose them from a table of constants fitted on two point loads at one image size (48 frames, a 49-96
    // sequence band, 65 536 point-frames ...), which sent every other shape wherever the table happened to put it.  Now
    // the first run of a new (mode, image size, frames, point-load) key PROBES the candidates on the caller's own data --
    // a batch run is idempotent, a lock-step step is re-run without its state-carrying kernels -- keeps the fastest and
    // remembers it for the process (tune_*).  vo_set_schedule() pins any knob instead.
    struct Schedule {
        int waves = 2, streams = 1, prep = 1;
        int wide = 4; // four-kernel EPnP for launches of up to this many frames (4 or 16; acts for 5 .. 16 frames per run)
        bool operator==(const Schedule &o) const { return waves == o.waves && streams == o.streams && prep == o.prep && wide == o.wide; }
        bool same_pair(const Schedule &o) const { return streams == o.streams && prep == o.prep; } // the two knobs dry runs misjudge
        vo_schedule abi() const { return vo_schedule{waves, streams, prep, wide}; }
        static Schedule from(const vo_schedule &s)
        {
            Schedule r;
            r.waves = s.pose_waves, r.streams = s.pose_streams, r.prep = s.prepare, r.wide = s.epnp_wide_frames;
            return r;
        }
    } sched;
    vo_schedule pin = {0, 0, -1, 0}; // 0 / 0 / -1 / 0 = probe
    long long sched_key[8] = {-1, 0, 0, 0, 0, 0, 0, 0}; // key `sched` was resolved for
    bool sched_probed = false;       // `sched` came out of a probe (here or earlier in the process), not from defaults
    bool tuning = false;             // inside a probe: run_stages must not start another one
    bool sync_call = false;          // the run being scheduled is a synchronous drop-in call (its own probe key: latency)
    // Lock-step loop: the comparison of schedules over REAL steps (capi_sched.hip: sched_before_step starts it, sched_after_step
    // drives it, sched_abandon drops it).  phase 1 = timing list[0] (the dry probe's pick), 2 = timing list[1], ... (cnt
    // candidates), cnt + 1 = decided; `left` counts down the phase's steps (VO_AB_RAMP untimed ramp steps + n timed).
    struct Compare {
        Schedule list[8]; // up to four nominees + (round 6, from 32 sequences on) every (pose_streams, prepare) pair once more
                          // with the OTHER register budget
        long long key[8] = {};
        int phase = 0, left = 0, n = 0, cnt = 0;
        bool extra = false;      // the twins with the other pose_waves have been appended
        hipEvent_t ev[16] = {};  // start / end of every candidate's timed window (events of the loop's configuration: Seq::own)
        bool running() const { return phase >= 1 && phase <= cnt; }
    } cmp;
    // what the last probe of this context measured: candidates and their steady-state ms per run (vo_get_probe_log; written
    // through probe_log_find / probe_log_record, capi_sched.hip)
    int probe_n = 0;
    vo_schedule probe_cand[VO_PROBE_LOG_MAX] = {};
    float probe_ms[VO_PROBE_LOG_MAX] = {};
    int probe_real[VO_PROBE_LOG_MAX] = {};          // 1: probe_ms[i] was (re)measured over real steps of the lock-step loop
    hipStream_t last_pose_stream = nullptr; // stream the latest pose chain was enqueued on
    bool quads_set = false; // d_quads holds h_quads (cleared whenever the table is zeroed)
    // synchronous drop-in calls (capi_dropin.hip): image slot of the LEFT image of the stereo pair the last vo_track_frame /
    // vo_circular_match received as its t1 pair (0 or 2; its right image follows it), pyramids built -- the next call may name it
    // as its t0 pair by passing no t0 images (main.cpp:157-158: imageLeft_t0 = imageLeft_t1).  -1: no such pair (no call yet,
    // or the batch / sequence API has touched the image table since)
    int tf_base = -1;
    // (round 6) The t1 pair of a synchronous drop-in call ON THE KEPT PAIR that single_frame_setup has NOT sent yet: hop 0 of
    // the LK chain reads the t0 pair only, so run_stages launches it first (lk_hops_kernel) and lets the t1 pair cross PCIe and
    // get its pyramids on the filter stream beside it; hops 1 .. 3 follow behind ev_t1_ready.  Host pointers of the caller: valid
    // inside the call that set them only -- vo_track_frame / vo_circular_match clear the record on every way out (DeferGuard).
    struct Deferred {
        int n = 0;                         // 2: img[0] / img[1] go to image slots first, first + 1
        const uint8_t *img[2] = {nullptr, nullptr};
        int first = 0, stride = 0;
    } defer;
    hipEvent_t ev_t1_ready = nullptr;
    // identity of that pair (vo_kept_pair_id): bumped whenever a drop-in call publishes a new t1 pair, so that a caller who
    // shares the context with others can tell whether the pair on the device is still the one ITS last call left
    int64_t tf_gen = 0;
    bool last_run_serial = true; // the last run_stages put everything on the tracking stream (else: sync_all before a gather)
    bool serial_pose = false; // developer build + VO_SERIAL_POSE=1 (vo_dev_hooks.h): the whole chain on the tracking stream (profiling)
    // pinned staging for host images: rows are repacked to the device pitch on the host and go over
    // PCIe as ONE contiguous copy (a pitched copy from pageable memory moves row by row: 3.3 ms per
    // 1241 x 376 image measured, tools/latency_mode.py)
    uint8_t *h_stage = nullptr, *d_stage = nullptr; // (d_stage: the same memory as the GPU addresses it, launch_pull_image)
    uint8_t *h_gather = nullptr, *d_gather = nullptr; // vo_track_frame's result buffer: host memory, and its device address
    uint8_t *d_pts_stage = nullptr; // (its device address)
    uint8_t *h_feat_stage = nullptr, *d_feat_stage = nullptr; // pinned + its device address: vo_detect_bucket's carried feature set on its way in (fcap float2 + fcap int32)
    uint8_t *h_pts_stage = nullptr; // pinned: the points + count of a synchronous drop-in call on their way to the device (cap float2 + 16 bytes)
    size_t stage_slot = 0; // bytes per slot, VO_STAGE_SLOTS slots
    // rectification at ingest (vo_params.rectify; all null in a context without maps): the packed maps of both sides, one raw
    // plane per staging slot (vo_rectify.h: zero frame written once, here), and THE table rectify_kernel reads -- entry i sends
    // raw plane i % VO_STAGE_SLOTS to image i with the maps of side i & 1.  An upload's pull and its rectify_kernel are ordered
    // on one stream, and all uploads between two drains go to one stream, so the planes need no signal of their own.
    uint32_t *d_rect_maps = nullptr;
    uint8_t *d_rect_raw = nullptr;
    RectImage *d_rect_tab = nullptr;
    size_t rect_plane = 0; // bytes per raw plane
    int stage_next = 0;
    int ransac_cap = 0;
    float h_P[24] = {};
    bool have_P = false;
    std::vector<int> h_npts;
    int *d_overflow = nullptr;     // [B] VO_STAGE_DETECT capacity flags (bit 0: feature list, bit 1: bucketed set)
    LkQueues lk_queues;            // the ticket counters of lk_circular_queue_kernel (two sets, zero at allocation) + the launch parity
    Quad *quads_cur = nullptr;     // the quad table the launches read: d_quads, or one phase of seq.d_quads
    std::vector<Quad> h_quads;     // host copy of d_quads (stale-pyramid check)
    std::vector<uint8_t> img_stale; // image re-uploaded since its pyramid was last built
    // ---- two-image tracker (voflow_*, include/vo_flow.h, capi_flow.hip): allocated by the first such call ----
    struct Flow {
        bool ready = false;
        Quad *d_pairs = nullptr;     // [max_frames] (prev, next) of voflow_batch_set_pairs as (l0, r0), then VO_FLOW_CONST_PAIRS
        float2 *d_next = nullptr;    // [B][cap]
        uint8_t *d_status = nullptr; // [B][cap]
        float *d_err = nullptr;      // [B][cap]
        float2 *d_out0 = nullptr, *d_out1 = nullptr; // [cap] survivors of deleteUnmatchFeatures (synchronous calls: one frame)
        int32_t *d_idx = nullptr;    // [cap]
        int *d_nout = nullptr;       // [1]
        std::vector<Quad> h_pairs;   // host copy of the pairs (stale-pyramid check)
        int n_pairs = 0;             // 0: no pairs set (or the table has been configured again since)
        int cfg[4] = {0, 0, 0, 0};   // n_images, w, h, n_frames of the table the pairs were set for
        std::vector<uint8_t> next_set; // [max_frames] the frame's d_next rows hold a guess or a run's results since the pairs were set
    } flow;
    // ---- Shi-Tomasi detector (vocorn_*, include/vo_corners.h, capi_corners.hip): allocated by the first such call, regrown when a
    // batch run covers more images than any before it ----
    struct Corn {
        int slots = 0;               // image slots the buffers below hold
        int kcap = 0;                // power of two >= fcap: the sort's length
        unsigned *d_ints = nullptr;  // [3][slots]: max_key, ncand, nout
        unsigned long long *d_keys = nullptr, *d_ckeys = nullptr; // [slots][kcap]
        int *d_status = nullptr;     // [slots][fcap]
        float2 *d_pts = nullptr;     // [slots][fcap]
        float *d_maps = nullptr;     // [slots][max_h * max_w] the quality maps (slot 0: vocorn_min_eigen_map's too)
        int run_first = 0, run_n = 0; // image range of the latest vocorn_batch_run (run_n = 0: none since the table was configured)
        int cfg[3] = {0, 0, 0};      // n_images, w, h of the table it ran on
    } corn;
    // ---- the frame loop's detector (vodet_*, include/vo_detector.h, capi_detector.hip): a CHECKED record ----
    vodet_params det = {VODET_FAST, {5000, 0.01, 5.0}, {3, 0, 0.04}};
    // ---- the frame loop's top-up under a mask of the carried points (votop_*, include/vo_topup.h, capi_topup.hip): a CHECKED record,
    // and one plane per frame with the table the kernels read them through -- from `own`, grown where the candidate buffers grow ----
    struct TopUp {
        votop_params prm = {VOTOP_OFF, 5};
        int slots = 0;                     // frames the planes below serve
        size_t plane_stride = 0;           // bytes from one plane to the next (max_w x max_h, rounded up to 16)
        uint8_t *d_planes = nullptr;       // [slots][plane_stride] rows tight (w bytes)
        const uint8_t **d_table = nullptr; // [slots] d_planes + f * plane_stride
        int ran = 0;                       // frames of the latest masked detection outside the lock-step loop (0: none)
        int cfg[3] = {0, 0, 0};            // n_images, w, h of the table it ran on
    } top;
    // ---- cv::FAST under a mask (vofm_*, include/vo_fast_mask.h, capi_fast_mask.hip): a CHECKED record; one plane per frame with the
    // table the kernels read them through, the unmasked list of an inline detection and the filtered list bucket_kernel's split form
    // reads -- from `own`, taken by the first run with the record on or the first vofm_detect / vofm_replenish ----
    struct FastMask {
        vofm_params prm = {VOFM_OFF, 5};
        int slots = 0;                     // frames the buffers below serve
        size_t plane_stride = 0;           // bytes from one plane to the next (max_w x max_h, rounded up to 16)
        uint8_t *d_planes = nullptr;       // [slots][plane_stride] rows tight (w bytes)
        const uint8_t **d_table = nullptr; // [slots] d_planes + f * plane_stride
        float2 *d_raw = nullptr;           // [slots][fcap] cv::FAST's unmasked list of an inline detection (the look-ahead's is Seq::d_corners)
        int *d_nraw = nullptr;             // [slots]
        float2 *d_filt = nullptr;          // [slots][fcap] the list under the mask
        int ran = 0;                       // frames of the latest masked detection of the loop outside vo_seq_* (0: none)
        int cfg[3] = {0, 0, 0};            // n_images, w, h of the table it ran on
    } fm;
    // ---- the detector's masks (vocmask_*, include/vo_corners_mask.h, capi_corners_mask.hip): allocated by the first such call ----
    struct CornMask {
        bool ready = false;
        // (entry max_images of each: the synchronous calls', so that they never touch what the batch calls set)
        uint8_t *d_masks = nullptr;        // [max_images + 1][max_w * max_h] the mask of image i, rows tight (w bytes)
        float2 *d_kept = nullptr;          // [max_images + 1][cap] the kept points of image i on their way to the disc kernel
        const uint8_t **d_table = nullptr; // [max_images + 1] what a run reads: the mask of image i, or null for an image without one
        std::vector<uint8_t> has;          // [max_images] host mirror of d_table: the image has a mask
        bool any = false;                  // some image has one (vo_batch_configure drops them all)
    } cmask;
    // ---- lock-step sequence loop (vo_seq_*): S sequences x 1 frame per step, state carried on the device ----
    struct Seq {
        bool on = false;
        Owner own; // everything allocated for this configuration (seq_free)
        int S = 0, ring = 0, max_steps = 0;
        long long step = 0;           // steps enqueued so far
        Quad *d_quads = nullptr;      // [ring][S]: phase r = (t0 in ring slot r, t1 in slot (r + 1) % ring)
        int *d_active = nullptr;      // [VO_SEQ_INFLIGHT][S]
        int *h_active = nullptr;      // pinned, same shape
        double *d_pose = nullptr;     // [S][16]
        double *d_traj = nullptr;     // [S][max_steps][VO_SEQ_ROW]
        SeqFrameInfo *d_info = nullptr; // [S][max_steps]
        int *d_rows = nullptr, *d_rows_carry = nullptr, *d_nages = nullptr; // [S]
        std::vector<uint8_t> pushed, had_prev; // pair pushed for the pending step / for the previous step
        std::vector<uint8_t> ever, gap;        // has had a pair since its reset / resumes after a pause (VO_SEQ_F_GAP)
        std::vector<int> h_rows;               // frames processed per sequence since its reset (host mirror of d_rows)
        bool broken = false;                   // a step failed after it had consumed its pairs: vo_seq_reset(-1) first
        hipEvent_t ev_upload = nullptr;
        Signal carry, integ;                // the latest seq_carry / the latest integration has run
        Signal slot_free[VO_SEQ_MAX_RING];  // the LK that read ring slot r as its t0 pair has finished
        Signal step_end[VO_SEQ_INFLIGHT];   // end of the step that used this slot of the per-step tables
        // pinned staging for pageable host images: two generations of [S][2] pitched level-0 images
        uint8_t *h_stage = nullptr;
        // (round 6) the device twin of the staging area: when EVERY sequence's pair of a step is pageable, the step's half of
        // h_stage -- one contiguous block -- crosses the link in ONE copy-engine transfer (57 GB/s, no shader involved:
        // nothing that runs beside it slows down) and the ingest kernel re-pitches it HBM to HBM
        uint8_t *d_stage = nullptr;
        int n_pageable = 0;             // pageable pairs among the pending step's n_ing
        size_t stage_img = 0;
        Signal stage_free[2]; // the ingest kernel has read that half of the staging area
        Signal detect;        // (round 6) the latest step's detection has run: a PCIe ingest starts behind it
        // "prepare" work of a step runs on the copy stream, off the tracking stream's critical path: ingest of the new pairs,
        // their pyramids, and FAST + non-maximum suppression of their LEFT images -- the corners the NEXT step's
        // appendNewFeatures needs (visualOdometry.cpp:95-101 detects on imageLeft_t0, i.e. on the pair that arrived one
        // step earlier).  Per step the tracking stream is left with: bucketing -> LK -> filter -> carry.
        // (whether the prepare stream is used is vo_ctx::sched.prep; ingest_stream() is the stream the step's ingest kernel
        // goes to: the prepare stream when it is, a plain copy stream when not)
        float2 *d_corners = nullptr;      // [ring][S][fcap] FAST corners of the left image in each ring slot
        int *d_ncorn = nullptr;           // [ring][S]
        hipEvent_t ev_pyr = nullptr;      // pyramids of the pending step built (prep stream)
        Signal fast[VO_SEQ_MAX_RING];     // corners of ring slot r ready (prep stream)
        bool have_corners[VO_SEQ_MAX_RING] = {}; // d_corners of ring slot r belongs to the pair now in that slot
        // (include/vo_topup.h) with the top-up on the look-ahead leaves the response MAPS of ring slot r here instead of corners, and
        // the step finishes the detection under the carried points' mask.  One set per ring slot: see DESIGN 3.16
        float *d_topmaps = nullptr;       // [ring][S][max_w * max_h], or null
        SeqIngest *h_ing = nullptr, *d_ing = nullptr; // [VO_SEQ_INFLIGHT][S] pairs pushed for a step (pinned / device)
        int n_ing = 0, n_active = 0;    // pairs pushed for / sequences active in the pending step
        // rectification at ingest (vo_params.rectify, else all null): the step's i-th pushed pair is ingested into raw planes
        // 2 i, 2 i + 1 -- by the step's ingest kernel, through a twin of its table whose image0 is 2 i -- and one rectify_kernel
        // launch on the same stream sends the 2 n_ing planes to their ring slots.  One set of 2 S planes: ingest and rectify of
        // consecutive steps are ordered on the ingest stream.
        uint8_t *d_raw = nullptr;
        SeqIngest *h_ing_raw = nullptr, *d_ing_raw = nullptr; // [VO_SEQ_INFLIGHT][S]
        RectImage *h_rect = nullptr, *d_rect = nullptr;       // [VO_SEQ_INFLIGHT][2 S]
        bool ing_pcie = false;          // a pair of the pending step lives in host memory (launch_seq_ingest: grid size)
        bool begun = false, staged = false;
    } seq;
};

#define VO_STAGE_SLOTS 4
// the quadruples of the synchronous drop-in calls, resident behind the context's own table (d_quads + max_frames) from
// vo_create on: a call selects one (use_const_quad) instead of uploading it -- the stateless frame loop alternates between
// a detection quadruple and a tracking quadruple twice per frame, and an upload is a copy plus a stream synchronisation
#define VO_CONST_QUADS 4
static const vo::Quad VO_CONST_QUAD_TABLE[VO_CONST_QUADS] = {{0, 1, 2, 3}, {2, 3, 0, 1}, {0, 0, 0, 0}, {2, 2, 2, 2}};

inline int fail(vo_ctx *ctx, int code, const char *msg)
{
    ctx->err = msg;
    return code;
}
inline int fail_hip(vo_ctx *ctx, const char *what, hipError_t e)
{
    ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return VO_ERR_HIP;
}
#define VO_HIP_TRY(ctx, call)                                                                         \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail_hip(ctx, #call, e_);                                                          \
    } while (0)

// the detection grid's bucket edge in pixels (vo_detect_params.bucket_size, 0 = a tenth of the image height)
inline int bucket_size(const vo_ctx *c) { return c->dprm.bucket_size > 0 ? c->dprm.bucket_size : c->h / 10; }
// register budget of the pose kernels for the stand-alone calls (vo_pnp_ransac, vo_essential_pose): nothing runs beside
// them, so the full 512 registers unless the caller pinned the other variant
inline int standalone_waves(const vo_ctx *c) { return c->pin.pose_waves ? c->pin.pose_waves : 1; }
inline void use_const_quad(vo_ctx *c, int k) // frame 0 of a one-frame configuration reads VO_CONST_QUAD_TABLE[k]
{
    c->quads_cur = c->d_quads + c->max_frames + k;
    c->h_quads[0] = VO_CONST_QUAD_TABLE[k];
    c->quads_set = false; // d_quads itself no longer says what h_quads says: the next vo_batch_set_quads uploads
}
// the current feature set (see vo_ctx::pts_sel)
inline float2 *cur_pts(vo_ctx *c) { return c->pts_sel < 0 ? c->d_pts : c->d_pts_det[c->pts_sel]; }
inline int *cur_npts(vo_ctx *c) { return c->pts_sel < 0 ? c->d_npts : c->d_npts_det[c->pts_sel]; }
inline int *cur_ages(vo_ctx *c) { return c->pts_sel < 0 ? c->d_ages : c->d_ages_det[c->pts_sel]; }
// the bytes of a source row of vo_params.input_format that are ever read or copied (ingest_bpp: vo_kernels.h): one plane of a
// two-byte interleave ends with its last pixel (the right plane of an interleaved frame starts at byte 1: byte 2 w of its last
// row is outside the frame)
inline size_t fmt_row_bytes(int fmt, int w) { return fmt == VO_FMT_GRAY8_X2 ? 2 * (size_t)w - 1 : (size_t)w * ingest_bpp(fmt); }

// the stream the lock-step loop's ingest kernel goes to (created by ensure_ingest_stream; set_sched keeps it in existence)
inline hipStream_t ingest_stream(const vo_ctx *c) { return c->sched.prep ? c->sel->prep : c->sel->copy; }
// frames the EPnP workspaces of a pose buffer set are allocated for
inline int epnp_ws_frames(const vo_ctx *c) { return c->max_frames < VO_EPNP_WS_MAX_FRAMES ? c->max_frames : VO_EPNP_WS_MAX_FRAMES; }
// the pair of timing events (indices into the VO_EV_PER_RUN events of a run) that brackets stage s of the timing order PYRAMID,
// DETECT, LK, FILTER, TRIANGULATE, PNP: run_stages records by it, the timed getters read by it
struct StageEvents {
    int start, end;
};
inline StageEvents stage_events(int s) { return {s == 1 ? VO_NUM_STAGES + 2 : s < 3 ? s : s + 1, s < 3 ? s + 1 : s + 2}; }
// a value out of a host-visible result buffer
template <typename T>
T peek(const uint8_t *p)
{
    T v;
    memcpy(&v, p, sizeof(T));
    return v;
}

constexpr int EM_MAX_ITERS = 1000; // maxIters of the findEssentialMat overload the reference calls (OpenCV 4.5)

/* ------------------------------------- schedule probe ------------------------------------ */

struct TuneKey {
    long long k[8];
    bool operator<(const TuneKey &o) const
    {
        for (int i = 0; i < 8; i++)
            if (k[i] != o.k[i])
                return k[i] < o.k[i];
        return false;
    }
};

// the point load a schedule was probed at, in half-octave buckets (1722 .. 2435 points share one): the single-frame
// drop-in calls see a slightly different count every frame and must not probe every time
inline int pts_bucket(long long pts) { return pts <= 0 ? 0 : (int)floor(2.0 * log2((double)pts) + 0.5); }

#define D2H(dst, src, bytes)                                                                           \
    do {                                                                                              \
        if ((dst) && (bytes) > 0)                                                                      \
            VO_HIP_TRY(c, hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, c->sel->stream)); \
    } while (0)

namespace vo_capi {
bool tuned_lookup(const TuneKey &key, vo_ctx::Schedule *s); // the per-process table of settled schedules (capi_sched.hip)
int plan_levels(vo_ctx *c, int w, int h);
bool acquire_streams(int device, StreamSet *out);
hipStream_t ensure_ingest_stream(vo_ctx *c, bool prepare);
bool ensure_partitioned_streams(StreamSet *s, int device);
int select_streams(vo_ctx *c, bool partitioned); // call with every stream idle
void release_streams(int device, const StreamSet &s);
void seq_free(vo_ctx *c);
// idle: the caller has just drained the tracking stream (a synchronous drop-in call); pts / n_pts: the call's points ride along
// on: the stream the pull kernel of an idle upload goes to (default: the tracking stream)
// plain: no rectification although the context has maps (vo_fast_detect)
int upload_image(vo_ctx *c, int idx, const void *src, int stride, hipMemcpyKind kind, bool idle = false, const float *pts = nullptr, int n_pts = -1,
                 hipStream_t on = nullptr, bool plain = false);
int rect_check_pack(vo_ctx *c, const vo_params *p, std::vector<uint32_t> *packed);
int rect_commit(vo_ctx *c, const vo_params *p, const std::vector<uint32_t> &packed);
int ensure_em(vo_ctx *c);
int run_stages(vo_ctx *c, int stages, bool timed, hipEvent_t *evs = nullptr, bool dry = false);
int sync_all(vo_ctx *c);
TuneKey tune_key(const vo_ctx *c, int stages);
void apply_pins(const vo_ctx *c, vo_ctx::Schedule *s);
bool all_pinned(const vo_ctx *c);
bool wide_knob_live(const vo_ctx *c);
int set_sched(vo_ctx *c, const vo_ctx::Schedule &s);
int sched_resolve(vo_ctx *c, int stages);
int sched_before_step(vo_ctx *c, int stages, hipEvent_t *evs);
int sched_after_step(vo_ctx *c, hipStream_t end_stream);
void sched_abandon(vo_ctx *c);
enum { SIG_STEP = 1, SIG_INGEST = 2, SIG_CHAIN = 4 };
void seq_forget(vo_ctx *c, int which);
int refuse_detect_shape(vo_ctx *c, const char *who, const char *what);
int seq_enqueue_inputs(vo_ctx *c, bool dry);
int seq_lookahead(vo_ctx *c, int r);
int probe_run(vo_ctx *c, int stages, bool timed, hipEvent_t *evs, bool dry);
int probe_candidate(vo_ctx *c, int stages, bool timed, hipEvent_t *evs, bool dry, bool latency, double *ms_per_run);
int tune_schedule(vo_ctx *c, int stages, bool timed, hipEvent_t *evs, bool dry, bool latency = false, bool publish = true);
int run_stages_auto(vo_ctx *c, int stages, bool timed, hipEvent_t *evs = nullptr, bool sync_call = false);
PnpParams pnp_params(const vo_ctx *c, const float *K = nullptr);
LkParams lk_params(const vo_ctx *c);
EmParams em_params(const vo_ctx *c);
bool have_kept_pair(const vo_ctx *c, int w, int h);
int deliver_pose(const vo_ctx *c, const PnpResult &r, const EmResult *e, double *rvec, double *tvec, double *R, bool pnp_rotation, bool io_pose);
int fail_overflow(vo_ctx *c, int ovf);
int fail_too_few_pnp(vo_ctx *c);
int get_pose_impl(vo_ctx *c, int frame, double *rvec, double *tvec, double *R, int32_t *inliers, int *n_inliers, int *status, int32_t *dbg4, bool pnp_rotation, int *em_status, bool io_pose = true);
int seq_begin_step(vo_ctx *c);
int seq_push(vo_ctx *c, int seq, const void *left, const void *right, int stride, int mode);
int single_frame_setup(vo_ctx *c, const uint8_t *l0, const uint8_t *r0, const uint8_t *l1, const uint8_t *r1, int w, int h, int stride, const float *pts, int n, bool defer_t1 = false);
int single_image_setup(vo_ctx *c, const uint8_t *img, int w, int h, int stride, bool plain = false);
int flush_deferred(vo_ctx *c, hipStream_t on);
// the Shi-Tomasi detector's host side (capi_corners.hip), shared with its masked calls (capi_corners_mask.hip) and with the calls that
// take a response (capi_corners_response.hip).  resp: a CHECKED record, or null for the 3 x 3 minimum eigenvalue -- the vocorn_* and
// vocmask_* entry points are these functions with resp == null, under their own names in `who`
int ensure_corn(vo_ctx *c, int slots);
vo::CornArgs corn_args(vo_ctx *c, const vocorn_params &p, const voresp_params *resp = nullptr);
int corn_check_params(vo_ctx *c, const char *who, const vocorn_params *in, vocorn_params *p);
int corn_sync_image(vo_ctx *c, const char *who, const uint8_t *img, int w, int h, int stride, int *image);
int corn_fetch(vo_ctx *c, const char *who, int s, float *pts_out, int cap, int *n_out);
int corn_detect(vo_ctx *c, const char *who, const uint8_t *img, int w, int h, int stride, const vocorn_params *params, const voresp_params *resp,
                float *pts_out, int cap, int *n_out);
int corn_map(vo_ctx *c, const char *who, const uint8_t *img, int w, int h, int stride, const voresp_params *resp, float *out, int out_stride_floats);
int corn_batch_run(vo_ctx *c, const char *who, const vocorn_params *params, int first_image, int n_images, bool masked,
                   const voresp_params *resp = nullptr);
int corn_check_resp(vo_ctx *c, const char *who, const voresp_params *in, voresp_params *r); // (capi_corners_response.hip)
// the frame loop under VODET_SHI_TOMASI (capi_detector.hip): the candidate buffers for `frames` frames (may drain the context: never
// inside a lock-step step), and the detector over the frames of `quads` into corners [frames][fcap] / n_out [frames] on `stream`
inline bool shi_tomasi(const vo_ctx *c) { return c->det.detector == VODET_SHI_TOMASI; }
// the top-up under a mask of the carried points acts (include/vo_topup.h): det_ensure then takes the planes too, det_launch runs the
// masked route, and the lock-step loop's look-ahead is det_lookahead_maps (the map pass alone, into ring slot r's maps) with
// det_launch(..., maps = that slot's) finishing it in the step
inline bool topup_on(const vo_ctx *c) { return shi_tomasi(c) && c->top.prm.mode == VOTOP_CARRIED; }
// cv::FAST's mask in the frame loop acts (include/vo_fast_mask.h): run_detect and vo_seq_configure take fm's buffers (fm_ensure) and
// the FAST route becomes list, discs, filter, split bucketing (fm_finish behind the unmasked list, wherever it was made)
inline bool fastmask_on(const vo_ctx *c) { return !shi_tomasi(c) && c->fm.prm.mode == VOFM_CARRIED; }
int fm_ensure(vo_ctx *c, int frames); // (capi_fast_mask.hip) may drain the context: never inside a lock-step step
// the discs of the detecting frames' carried points and the filter of raw [frames][fcap] / n_raw [frames] under them, into fm.d_filt
// and d_nnew, on `stream`
int fm_finish(vo_ctx *c, const int *d_detect, int frames, const float2 *raw, const int *n_raw, hipStream_t stream);
int det_ensure(vo_ctx *c, int frames);
int top_ensure(vo_ctx *c, int frames); // (capi_topup.hip) the planes and their table for `frames` frames; may drain the context
int det_launch(vo_ctx *c, const vo::Quad *quads, const int *d_detect, int frames, float2 *corners, int *n_out, hipStream_t stream,
               const float *ahead_maps = nullptr);
int det_lookahead_maps(vo_ctx *c, const vo::Quad *quads, int frames, float *maps, hipStream_t stream);
int cmask_detect(vo_ctx *c, const char *who, const uint8_t *img, int w, int h, int stride, const uint8_t *mask, int mask_stride,
                 const vocorn_params *params, const voresp_params *resp, float *pts_out, int cap, int *n_out); // (capi_corners_mask.hip)
struct DeferGuard { // the deferred t1 pair never outlives the call whose host pointers it holds
    vo_ctx *c;
    ~DeferGuard() { c->defer.n = 0; }
};
} // namespace vo_capi

using namespace vo_capi;
