// vo_corners_dev.h -- what corners.hip (the Shi-Tomasi detector's kernels), its host code capi_corners.hip and the CPU emulator
// harness of the tests share: the argument record of the kernels and their launch wrapper.
#pragma once
#include "vo_dev.h"

#include <string.h>

namespace vo {

// One run over n image slots (slot s = image `first + s` of the image table).  Every per-slot array is indexed by the slot.
struct CornArgs {
    unsigned *max_key;         // [n] ordered bits (corn_ord) of the quality map's maximum; 0 before the run
    int *ncand;                // [n] candidates that passed the threshold (may exceed lcap: nothing beyond it is stored); 0 before
    int *nout;                 // [n] corners found, -1: the candidate list overflowed (frames form: lcap + 1)
    int *rounds;               // [n] rounds the suppression took, or null (the library does not ask; the emulator harness does)
    float *maps;               // [n][map_stride] the quality maps, rows tight (w floats)
    size_t map_stride;
    unsigned long long *keys;  // [n][kcap] candidates as (corn_ord(quality) << 32 | y * w + x), sorted descending by the select kernel
    unsigned long long *ckeys; // [n][kcap] (cell << 32 | rank), ascending
    int *status;               // [n][lcap] 0 undecided, else round << 1 | accepted
    float2 *pts;               // [n][lcap] the corners, best first
    int lcap, kcap;            // list capacity; kcap = the power of two >= lcap
    double quality;            // qualityLevel
    int max_corners;           // <= 0: no limit
    int cell;                  // cvRound(minDistance), >= 1
    int lim;                   // two candidates of neighbouring cells conflict iff dx^2 + dy^2 < lim (= ceil(minDistance^2)); <= 1: none can
    // goodFeaturesToTrack's mask argument (include/vo_corners_mask.h).  As initialised here: no mask, and the run is what it was.
    const uint8_t *const *masks = nullptr; // [n] the slot's mask (h rows of w bytes, mask_pitch bytes apart; non-zero: allowed), or
                                           // null for a slot without one.  A null table: no slot has one
    int mask_pitch = 0;
    // goodFeaturesToTrack's blockSize, useHarrisDetector and k (include/vo_corners_response.h).  As initialised here: the 3 x 3
    // minimum eigenvalue through corn_map_kernel / corn_map_masked_kernel, and the run is what it was.
    int block_size = 3;   // 3 or 5
    int use_harris = 0;   // 0: calcMinEigenVal, 1: calcHarris
    double harris_k = 0.04;
};

// A float's bits as an unsigned that orders like the float (negative values included): the map maximum by atomicMax, the sort key
__host__ __device__ inline unsigned corn_ord(float v)
{
    unsigned u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float corn_unord(unsigned k)
{
    const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float v;
    memcpy(&v, &u, 4);
    return v;
}
inline int corn_pow2(int n)
{
    int p = 1;
    while (p < n)
        p <<= 1;
    return p;
}

// what the top-up's masked route takes beside CornArgs (include/vo_topup.h; launch_corners_frames_masked below)
struct CornTopArgs {
    const float2 *feat;     // [n][fcap] the frames' feature lists: the carried points first
    int fcap;
    const int *n_tracked;   // [n] carried points per frame, on the device
    int radius;
    uint8_t *const *planes; // [n] device table of the planes (what a.masks reads)
    uint8_t *plane0;        // plane 0; plane f lies plane_stride bytes further on, rows w bytes apart
    size_t plane_stride;
    int max_kept;           // the largest carried set that still detects again (sizes the disc grid)
};

#ifndef VO_HOST_EMUL
// the whole detector over n slots: map + maximum, candidates, sort + suppression + output (three launches on `stream`; max_key and
// ncand are zeroed first).  Returns the first HIP error of the memsets and launches.  With a.masks the map pass is the masked twin;
// with a.block_size / a.use_harris other than (3, 0) it is corn_map_resp_kernel<block_size, use_harris>, masked or not.
hipError_t launch_corners(const PyrImage *d_imgs, int first, int n, int w, int h, const CornArgs &a, hipStream_t stream);
// The same three passes in the FRAMES form (the frame loop, include/vo_detector.h): slot = frame, image = d_quads[frame].l0, and
// d_detect (null: every frame) the frames' "detect again" flags on the device.  a.pts / a.nout point at the loop's own corner list
// [n][a.lcap] and count [n] (bucket_kernel's split form reads them); a frame that does not detect gets nout = 0, a candidate list
// beyond a.lcap nout = a.lcap + 1 (which bucket_kernel reports as the frame's list overflow).  a.masks is not read.
hipError_t launch_corners_frames(const PyrImage *d_imgs, const Quad *d_quads, const int *d_detect, int n, int w, int h, const CornArgs &a,
                                 hipStream_t stream);
// The frame loop's top-up under a mask of the carried points (include/vo_topup.h) is the frames form in two parts, so that the
// lock-step loop's look-ahead can run the first before the step's carried sets exist:
//   launch_corners_frames_map     the map pass alone into a.maps (no maximum: max_key is not written)
//   launch_corners_frames_masked  0xFF over the n planes, the discs of every detecting frame's carried points (corn_disc_frames_kernel),
//                                 the maximum of the stored map under the plane (corn_max_frames_kernel), then the candidate pass under
//                                 a.masks (= the plane table, a.mask_pitch = w) and the select pass; max_key and ncand are zeroed first
hipError_t launch_corners_frames_map(const PyrImage *d_imgs, const Quad *d_quads, const int *d_detect, int n, int w, const CornArgs &a, hipStream_t stream);
hipError_t launch_corners_frames_masked(const int *d_detect, int n, int w, int h, const CornArgs &a, const CornTopArgs &t, hipStream_t stream);
// its first step alone -- 0xFF over the n planes and the discs of every detecting frame's carried points -- which cv::FAST's mask in
// the frame loop (include/vo_fast_mask.h) shares with it
hipError_t launch_corner_disc_frames(const int *d_detect, int n, int w, int h, const CornTopArgs &t, hipStream_t stream);
// cv::cornerMinEigenVal(img, map, block_size, 3) or cv::cornerHarris(img, map, block_size, 3, k) of image `image` into map [h][w]
// (tight); block_size 3 or 5
void launch_corner_map(const PyrImage *d_imgs, int image, int w, int h, float *d_map, hipStream_t stream, int block_size = 3, int use_harris = 0,
                       double k = 0.04);
// the disc mask of include/vo_corners_mask.h into mask [h][w] (tight): 0xFF everywhere, then 0 within `radius` of every kept point
// (a memset and, with n_kept > 0, one launch on `stream`)
hipError_t launch_corner_disc_mask(const float2 *d_kept, int n_kept, int radius, uint8_t *d_mask, int w, int h, hipStream_t stream);
#endif

} // namespace vo
