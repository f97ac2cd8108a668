// dev/capi_dev.hip -- the entry points only libvo_hip_dev.so has (python -m visual_odom_amd.build --dev): the time stamps of the
// developer build, read by tools/pose_phases.py and tools/host_gap_probe.py.
#include "../capi_internal.h"

// host-side time stamps of the last vo_track_frame (ns, steady clock; VO_HOST_STAMP in capi_dropin.hip): [0] entry, [1] configure +
// sync_all done, [2..5] image k staged and its copy enqueued, [6] points enqueued, [7] run_stages returned (everything
// enqueued), [8] the final stream synchronisation returned, [9] results copied out
long long g_host_stamp[16];

namespace vo {
int pose_prof_read(long long *out64); // dev/pnp_dev.hip
}

extern "C" {

int vo_dev_host_stamps(long long *out16)
{
    if (!out16)
        return VO_ERR_ARG;
    memcpy(out16, g_host_stamp, sizeof(g_host_stamp));
    return VO_OK;
}

// the 100 MHz stamps the pose kernels left for frame 0 / hypothesis 0
int vo_dev_pose_prof(vo_ctx *c, long long *out64)
{
    if (!c || !out64 || vo_capi::sync_all(c) != VO_OK)
        return VO_ERR_ARG;
    return vo::pose_prof_read(out64) == 0 ? VO_OK : VO_ERR_HIP;
}

} // extern "C"
