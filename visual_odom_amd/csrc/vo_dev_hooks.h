// vo_dev_hooks.h -- what the developer build (python -m visual_odom_amd.build --dev -> libvo_hip_dev.so, -DVO_DEV_VARIANTS) hooks
// into the product sources: tuning switches read from the environment and time stamps.  In the product build every hook is a
// constant or expands to nothing, and the library reads no environment variable.  Besides the two launch branches of the slim
// pose chain in pnp.hip this is the only file outside csrc/dev/ that tests VO_DEV_VARIANTS; the kernel variants of the
// developer build and the switches that select them live in csrc/dev/.
#pragma once

#ifdef VO_DEV_VARIANTS
#include <chrono>
#include <stdlib.h>

// a tuning switch: the integer value of the environment variable, `dflt` where it is not set
inline int dev_knob(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
// pose_waves values vo_set_schedule takes: 4 = the slim pose chain (pnp.hip), measured slower everywhere, kept for the record
constexpr int VO_DEV_MAX_POSE_WAVES = 4;

// host-side time stamps of the last vo_track_frame (dev/capi_dev.hip, vo_dev_host_stamps)
extern long long g_host_stamp[16];
#define VO_HOST_STAMP(k) \
    (g_host_stamp[k] = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count())

// 100 MHz time stamps of one EPnP hypothesis / one refinement into g_pose_prof (dev/pnp_dev.hip, tools/pose_phases.py);
// VO_POSE_PROF(...): bookkeeping statements of select_refine_kernel that exist in the developer build only
#ifdef __HIP_DEVICE_COMPILE__
#define VO_EPNP_STAMP(i)                                                      \
    do {                                                                      \
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {         \
            g_pose_prof[i] = (long long)wall_clock64();                       \
        }                                                                     \
    } while (0)
#define VO_POSE_NOW() ((long long)wall_clock64())
#else
#define VO_EPNP_STAMP(i)
#define VO_POSE_NOW() 0ll
#endif
#define VO_POSE_PROF(...) __VA_ARGS__

#else // the product

constexpr int dev_knob(const char *, int dflt) { return dflt; }
constexpr int VO_DEV_MAX_POSE_WAVES = 2;
#define VO_HOST_STAMP(k) ((void)0)
#define VO_EPNP_STAMP(i)
#define VO_POSE_PROF(...)

#endif
