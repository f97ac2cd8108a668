// dev/pnp_dev.hip -- pnp.hip with the buffer its time stamps go to.
//
// The developer build (python -m visual_odom_amd.build --dev -> libvo_hip_dev.so) compiles this file INSTEAD of pnp.hip: the stamp
// macros of vo_dev_hooks.h write into g_pose_prof, which has to live in the translation unit of the kernels.
#include "../vo_kernels.h"

// [0 .. 8] epnp_kernel, hypothesis 0 of frame 0 (vo_epnp.h); [16 ..] select_refine_kernel, thread 0 of frame 0 (pnp.hip)
__device__ long long g_pose_prof[64];

#include "../pnp.hip"

namespace vo {

int pose_prof_read(long long *out64)
{
    return hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_pose_prof), sizeof(long long) * 64) == hipSuccess ? 0 : -1;
}

} // namespace vo
