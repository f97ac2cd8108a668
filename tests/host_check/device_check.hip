// device_check.hip -- TEST ONLY: the unit vectors of the VO_HD device-math headers run ON gfx950.  A filter: operands in,
// device results out.  It holds no references and makes no judgement; tests/test_gpu_device_units.py compiles it with hipcc
// (the product's flags), runs it once and compares its outputs with the g++ build of the same headers (host_check.cpp) bit
// for bit and with high-precision references.  Not a product path: libvo_hip never links this.
//
//     device_check [--host] <dir>
//
// For every operation `op` below, if <dir>/<op>.in exists it holds n records of IN bytes each (raw little-endian, fields
// at their natural alignment; n = file size / IN), and <dir>/<op>.out receives n records of OUT bytes.  Operations without a
// file are skipped.  Prints "OK <op> <op> ..." and exits 0; a HIP error or a file of the wrong size prints "FAIL: ..." and
// exits non-zero at once, launching nothing further.
//
// One thread per case (records: tests/host_check/unit_cases.h, which also names the operations):
//     math_cbrt math_acos math_cos math_sin math_lambda                                         f64 -> f64
//     epnp5 p3p4 p3p_deg4 rodrigues_v2m rodrigues_m2v triangulate five_point sampson decompose cheirality solve6 svd12
//     lk_perm_b32 lk_udot2 lk_sdot2 lk_sdot2_first lk_pk_sub_i16 lk_pk_lshr1_u16 lk_udot4 lk_pk_add_u16 lk_pk_subsat_u16
//     lk_pk_min_u16 lk_pk_mad_u16 lk_alignbyte lk_pack_w                                        u32 a, b, c -> u32
//     lk_bilinear7_u8 lk_blend7 lk_bilinear7_deriv lk_diff_dot lk_scharr4
// Wide routines (device only):
//     svd12_wide     f64 At[144] -> f64 rows[144]: a 128-thread workgroup per matrix in LDS, jacobi12_pipe_sweeps +
//                    jacobi12_finish on thread 0, as svd12_wave_kernel
//     solve6_wave1   f64 A[36], b[6] -> f64 x[6]: one wavefront per workgroup (jacobi6v_wave_sweeps, then jacobi_finish<6, true>
//                    + svd_backsubst<6> on lane 0)
//     solve6_wave4   the same records by 256-thread workgroups: each of the four wavefronts solves a system of its own in its
//                    own LDS slice, no workgroup barrier between them (select_refine_kernel's use)
//     row_sums       f64 x6[64], y6[64], x12[64], y12[64] (one value per lane of a wavefront) -> f64 [2][6][64]: per lane
//                    row_ordered_sum<6>(x6), row_ordered_sum<12>(x12), row_ordered_sum_x2<6>(x6, y6) (two outputs),
//                    row_ordered_sum_x2<12>(x12, y12) (two) -- [0]: all four DPP rows active; [1]: the operands swapped
//                    (y for x), inside a branch only rows 1 and 3 take, rows 0 and 2 keep ROW_SUMS_SENTINEL
//     epnp_split     the record of epnp5 -> f64 rvec[3], tvec[3] through the four kernels of pnp.hip: epnp5_prepare<64> (LDS,
//                    lane-interleaved) | wide SVD | epnp5_L_rho<1> + epnp5_approx<1, a> (a = blockIdx.z) | epnp5_select
//     fast_pair      i32 max_tuples -> u64 disagreements, u64 comparisons, then max_tuples x u32 {v, c0, c4, c8, c12, t2,
//                    result, wanted lane bits}: fast_compass_pair against fast_compass_candidate over the sweep of
//                    ke_fast_compass_pair_check (kernel_emu.cpp), generated on the device
// --host runs the host side of the one-thread-per-case operations (the `#else` branches, compiled by the host pass of hipcc)
// without touching the HIP runtime; the wide routines and fast_pair (fast.hip's functions are __device__ only) have none.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../visual_odom_amd/csrc/vo_dev.h"
#include "../../visual_odom_amd/csrc/fast.hip"
#include "../../visual_odom_amd/csrc/vo_svd_wide.h"
#include "unit_cases.h"

#define ROW_SUMS_SENTINEL (-7.0)

static void fail(const char *what, const char *detail)
{
    printf("FAIL: %s: %s\n", what, detail);
    fflush(stdout);
    exit(2);
}
#define HIP_OK(call)                                   \
    do {                                               \
        const hipError_t e_ = (call);                  \
        if (e_ != hipSuccess)                          \
            fail(#call, hipGetErrorString(e_));        \
    } while (0)

// ---- files ---------------------------------------------------------------------------------------------------------
static std::string g_dir, g_done;
static bool load(const char *op, size_t record, std::vector<char> &buf)
{
    const std::string path = g_dir + "/" + op + ".in";
    FILE *f = fopen(path.c_str(), "rb");
    if (!f)
        return false;
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (size < 0 || (size_t)size % record != 0)
        fail(path.c_str(), "size is no multiple of the record");
    buf.resize((size_t)size);
    if (size && fread(buf.data(), 1, (size_t)size, f) != (size_t)size)
        fail(path.c_str(), "short read");
    fclose(f);
    return true;
}
static void store(const char *op, const void *data, size_t bytes)
{
    const std::string path = g_dir + "/" + op + ".out";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || (bytes && fwrite(data, 1, bytes, f) != bytes) || fclose(f) != 0)
        fail(path.c_str(), "cannot write");
    g_done += std::string(" ") + op;
}
// device copies of one operation's records: in -> device, zeroed out; after the launch: synchronise, check, fetch, store
struct DevIo {
    char *din = nullptr, *dout = nullptr;
    std::vector<char> out;
    DevIo(const std::vector<char> &in, size_t out_bytes) : out(out_bytes)
    {
        HIP_OK(hipMalloc((void **)&din, in.size() ? in.size() : 1));
        HIP_OK(hipMalloc((void **)&dout, out_bytes ? out_bytes : 1));
        HIP_OK(hipMemcpy(din, in.data(), in.size(), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(dout, 0, out_bytes));
    }
    void finish(const char *op)
    {
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out.data(), dout, out.size(), hipMemcpyDeviceToHost));
        HIP_OK(hipFree(din));
        HIP_OK(hipFree(dout));
        store(op, out.data(), out.size());
    }
};

// ---- one thread per case ---------------------------------------------------------------------------------------------
template <class Op>
__global__ __launch_bounds__(64) void case_kernel(const char *__restrict__ in, char *__restrict__ out, int n)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n)
        Op::run(in + (size_t)i * Op::IN, out + (size_t)i * Op::OUT);
}
template <class Op>
static void run_case(bool host)
{
    std::vector<char> in;
    if (!load(Op::name(), Op::IN, in))
        return;
    const int n = (int)(in.size() / Op::IN);
    if (host) {
        std::vector<char> out((size_t)n * Op::OUT);
        for (int i = 0; i < n; i++)
            Op::run(in.data() + (size_t)i * Op::IN, out.data() + (size_t)i * Op::OUT);
        store(Op::name(), out.data(), out.size());
        return;
    }
    DevIo io(in, (size_t)n * Op::OUT);
    if (n)
        hipLaunchKernelGGL(case_kernel<Op>, dim3((n + 63) / 64), dim3(64), 0, 0, io.din, io.dout, n);
    io.finish(Op::name());
}
template <class... Ops>
static void run_cases(uc::OpList<Ops...>, bool host)
{
    (run_case<Ops>(host), ...);
}

// ---- the wide routines ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void svd12_wide_kernel(const double *__restrict__ in, double *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) double s_at[144];
    __shared__ double s_w[12];
    __shared__ int s_flag;
    const int tid = threadIdx.x;
    const size_t q = blockIdx.x;
    for (int i = tid; i < 144; i += 128)
        s_at[i] = in[q * 144 + i];
    __syncthreads();
    vo::jacobi12_pipe_sweeps(s_at, s_w, &s_flag, tid);
    __syncthreads();
    if (tid == 0)
        vo::jacobi12_finish(s_at, s_w);
    __syncthreads();
    for (int i = tid; i < 144; i += 128)
        out[q * 144 + i] = s_at[i];
}

// WAVES wavefronts per workgroup, each with a system and an LDS slice of its own; nothing but wavefront-level ordering
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void solve6_wave_kernel(const double *__restrict__ in, double *__restrict__ out, int n)
{
    __shared__ double s_at[WAVES][36], s_vt[WAVES][36], s_w[WAVES][6];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, q = blockIdx.x * WAVES + wv;
    if (q >= n) // (uniform over the wavefront)
        return;
    const double *A = in + (size_t)q * 42, *b = A + 36;
    if (lane == 0)
        for (int i = 0; i < 6; i++)
            for (int k = 0; k < 6; k++)
                s_at[wv][i * 6 + k] = A[k * 6 + i];
    vo::wide_sync(true);
    vo::jacobi6v_wave_sweeps(s_at[wv], s_w[wv], s_vt[wv], lane);
    vo::wide_sync(true);
    if (lane == 0) {
        double x[6];
        vo::jacobi_finish<6, true>(s_at[wv], s_w[wv], s_vt[wv]);
        vo::svd_backsubst<6>(s_at[wv], s_w[wv], s_vt[wv], b, x);
        for (int k = 0; k < 6; k++)
            out[(size_t)q * 6 + k] = x[k];
    }
}

__global__ __launch_bounds__(64) void row_sums_kernel(const double *__restrict__ in, double *__restrict__ out)
{
    const int lane = threadIdx.x, row = lane >> 4;
    const double *p = in + (size_t)blockIdx.x * 256;
    double *o = out + (size_t)blockIdx.x * 768;
    const double x6 = p[lane], y6 = p[64 + lane], x12 = p[128 + lane], y12 = p[192 + lane];
    double r[6];
    r[0] = vo::row_ordered_sum<6>(x6);
    r[1] = vo::row_ordered_sum<12>(x12);
    vo::row_ordered_sum_x2<6>(x6, y6, r[2], r[3]);
    vo::row_ordered_sum_x2<12>(x12, y12, r[4], r[5]);
#pragma unroll
    for (int k = 0; k < 6; k++)
        o[k * 64 + lane] = r[k];
#pragma unroll
    for (int k = 0; k < 6; k++)
        r[k] = ROW_SUMS_SENTINEL;
    if (row & 1) { // EXEC partly off, as in the sweeps (a DPP row's branch)
        r[0] = vo::row_ordered_sum<6>(y6);
        r[1] = vo::row_ordered_sum<12>(y12);
        vo::row_ordered_sum_x2<6>(y6, x6, r[2], r[3]);
        vo::row_ordered_sum_x2<12>(y12, x12, r[4], r[5]);
    }
#pragma unroll
    for (int k = 0; k < 6; k++)
        o[(6 + k) * 64 + lane] = r[k];
}

// the four-kernel EPnP; workspace per case: Epnp5 (88 doubles) | At 144 | 3 x (rep, R[9], t[3])
constexpr int WS = 88 + 144 + 39, WS_AT = 88, WS_RES = 232;
static_assert(sizeof(vo::Epnp5) == 88 * sizeof(double), "workspace layout");
__global__ __launch_bounds__(64, 1) void split_prepare_kernel(const float *__restrict__ in, double *__restrict__ ws, int n)
{
    extern __shared__ __attribute__((aligned(16))) double s_ut[]; // 144 x 64, lane-interleaved
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n)
        return;
    const float *f = in + (size_t)q * 34;
    float x5[15], u5[10], K[9];
    for (int i = 0; i < 15; i++)
        x5[i] = f[i];
    for (int i = 0; i < 10; i++)
        u5[i] = f[15 + i];
    for (int i = 0; i < 9; i++)
        K[i] = f[25 + i];
    double *w = ws + (size_t)q * WS;
    vo::Epnp5 e;
    vo::epnp5_prepare<64>(x5, u5, K, e, s_ut + threadIdx.x);
    *(vo::Epnp5 *)w = e;
    for (int i = 0; i < 144; i++)
        w[WS_AT + i] = s_ut[i * 64 + threadIdx.x];
}
__global__ __launch_bounds__(128) void split_svd_kernel(double *__restrict__ ws)
{
    __shared__ __attribute__((aligned(16))) double s_at[144];
    __shared__ double s_w[12];
    __shared__ int s_flag;
    const int tid = threadIdx.x;
    double *w = ws + (size_t)blockIdx.x * WS + WS_AT;
    for (int i = tid; i < 144; i += 128)
        s_at[i] = w[i];
    __syncthreads();
    vo::jacobi12_pipe_sweeps(s_at, s_w, &s_flag, tid);
    __syncthreads();
    if (tid == 0)
        vo::jacobi12_finish(s_at, s_w);
    __syncthreads();
    if (tid < 48) // rows 8 .. 11: the null-space basis is all the rest of the solver reads
        w[96 + tid] = s_at[96 + tid];
}
__global__ __launch_bounds__(64, 1) void split_approx_kernel(double *__restrict__ ws, int n)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n)
        return;
    double *w = ws + (size_t)q * WS;
    vo::Epnp5 e = *(const vo::Epnp5 *)w;
    const double *ut = w + WS_AT;
    double L[60], rho[6], R[9], t[3], rep;
    vo::epnp5_L_rho<1>(e, ut, L, rho);
    if (blockIdx.z == 0)
        rep = vo::epnp5_approx<1, 0>(e, ut, L, rho, R, t);
    else if (blockIdx.z == 1)
        rep = vo::epnp5_approx<1, 1>(e, ut, L, rho, R, t);
    else
        rep = vo::epnp5_approx<1, 2>(e, ut, L, rho, R, t);
    double *o = w + WS_RES + 13 * blockIdx.z;
    o[0] = rep;
    for (int k = 0; k < 9; k++)
        o[1 + k] = R[k];
    for (int k = 0; k < 3; k++)
        o[10 + k] = t[k];
}
__global__ __launch_bounds__(64) void split_select_kernel(const double *__restrict__ ws, double *__restrict__ out, int n)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n)
        return;
    const double *o = ws + (size_t)q * WS + WS_RES;
    double rep[3], R[3][9], t[3][3];
    for (int a = 0; a < 3; a++) {
        rep[a] = o[13 * a];
        for (int k = 0; k < 9; k++)
            R[a][k] = o[13 * a + 1 + k];
        for (int k = 0; k < 3; k++)
            t[a][k] = o[13 * a + 10 + k];
    }
    vo::epnp5_select(rep, R[0], R[1], R[2], t[0], t[1], t[2], out + (size_t)q * 6, out + (size_t)q * 6 + 3);
}

// fast_compass_pair against fast_compass_candidate: workgroup (x: centre index, y: threshold index), threads over the 9^4
// choices of the four compass pixels.  res[0] = disagreements, res[1] = comparisons; tuples: the first max_tuples of them
__global__ __launch_bounds__(256) void fast_pair_kernel(const int *__restrict__ centres, unsigned long long *__restrict__ res,
                                                        uint32_t *__restrict__ tuples, int max_tuples)
{
    const int thresholds[8] = {0, 1, 7, 20, 100, 200, 254, 255};
    const int threshold = thresholds[blockIdx.y], v0 = centres[blockIdx.x], v1 = (v0 * 7 + 13) & 255; // the other lane's centre
    const int stride = 7;
    int cand[2][9];
    for (int l = 0; l < 2; l++) {
        const int v = l ? v1 : v0;
        const int raw[9] = {0, 255, v, v + threshold, v + threshold + 1, v - threshold, v - threshold - 1, v + threshold - 1, v - threshold + 1};
        for (int k = 0; k < 9; k++)
            cand[l][k] = raw[k] < 0 ? 0 : raw[k] > 255 ? 255 : raw[k];
    }
    unsigned long long bad = 0, done = 0;
    for (int code = threadIdx.x; code < 9 * 9 * 9 * 9; code += 256) {
        uint8_t patch[2][7 * 7];
        uint32_t c[4] = {0, 0, 0, 0};
        bool want[2];
        for (int l = 0; l < 2; l++) {
            for (int i = 0; i < 49; i++)
                patch[l][i] = 0;
            const int k0 = code % 9, k4 = code / 9 % 9, k8 = code / 81 % 9, k12 = (code / 729 + 3 * l) % 9;
            const int px[4] = {cand[l][k0], cand[l][k4], cand[l][k8], cand[l][k12]};
            uint8_t *p = &patch[l][3 * stride + 3];
            p[0] = (uint8_t)(l ? v1 : v0);
            p[3 * stride] = (uint8_t)px[0];
            p[3] = (uint8_t)px[1];
            p[-3 * stride] = (uint8_t)px[2];
            p[-3] = (uint8_t)px[3];
            want[l] = vo::fast_compass_candidate(p, stride, threshold);
            for (int k = 0; k < 4; k++)
                c[k] |= (uint32_t)px[k] << (16 * l);
        }
        const uint32_t v = (uint32_t)v0 | (uint32_t)v1 << 16, t2 = (uint32_t)threshold | (uint32_t)threshold << 16;
        const uint32_t r = vo::fast_compass_pair(v, c[0], c[1], c[2], c[3], t2);
        const int wrong = (((r & 0xffffu) != 0) != want[0]) + (((r >> 16) != 0) != want[1]);
        done += 2;
        if (wrong) {
            bad += wrong;
            const unsigned long long slot = atomicAdd(&res[2], 1ull);
            if (slot < (unsigned long long)max_tuples) {
                uint32_t *t = tuples + 8 * slot;
                t[0] = v;
                for (int k = 0; k < 4; k++)
                    t[1 + k] = c[k];
                t[5] = t2;
                t[6] = r;
                t[7] = (uint32_t)want[0] | (uint32_t)want[1] << 1;
            }
        }
    }
    atomicAdd(&res[0], bad);
    atomicAdd(&res[1], done);
}

static void run_wide()
{
    std::vector<char> in;
    if (load("svd12_wide", 144 * 8, in)) {
        const int n = (int)(in.size() / (144 * 8));
        DevIo io(in, in.size());
        if (n)
            hipLaunchKernelGGL(svd12_wide_kernel, dim3(n), dim3(128), 0, 0, (const double *)io.din, (double *)io.dout);
        io.finish("svd12_wide");
    }
    if (load("solve6_wave1", 42 * 8, in)) {
        const int n = (int)(in.size() / (42 * 8));
        DevIo io(in, (size_t)n * 48);
        if (n)
            hipLaunchKernelGGL(solve6_wave_kernel<1>, dim3(n), dim3(64), 0, 0, (const double *)io.din, (double *)io.dout, n);
        io.finish("solve6_wave1");
    }
    if (load("solve6_wave4", 42 * 8, in)) {
        const int n = (int)(in.size() / (42 * 8));
        DevIo io(in, (size_t)n * 48);
        if (n)
            hipLaunchKernelGGL(solve6_wave_kernel<4>, dim3((n + 3) / 4), dim3(256), 0, 0, (const double *)io.din, (double *)io.dout, n);
        io.finish("solve6_wave4");
    }
    if (load("row_sums", 256 * 8, in)) {
        const int n = (int)(in.size() / (256 * 8));
        DevIo io(in, (size_t)n * 768 * 8);
        if (n)
            hipLaunchKernelGGL(row_sums_kernel, dim3(n), dim3(64), 0, 0, (const double *)io.din, (double *)io.dout);
        io.finish("row_sums");
    }
    if (load("epnp_split", 34 * 4, in)) {
        const int n = (int)(in.size() / (34 * 4));
        DevIo io(in, (size_t)n * 48);
        double *ws = nullptr;
        HIP_OK(hipMalloc((void **)&ws, sizeof(double) * WS * (n ? n : 1)));
        HIP_OK(hipMemset(ws, 0, sizeof(double) * WS * (n ? n : 1)));
        if (n) {
            const int g = (n + 63) / 64;
            hipLaunchKernelGGL(split_prepare_kernel, dim3(g), dim3(64), 144 * 64 * sizeof(double), 0, (const float *)io.din, ws, n);
            HIP_OK(hipGetLastError());
            hipLaunchKernelGGL(split_svd_kernel, dim3(n), dim3(128), 0, 0, ws);
            hipLaunchKernelGGL(split_approx_kernel, dim3(g, 1, 3), dim3(64), 0, 0, ws, n);
            hipLaunchKernelGGL(split_select_kernel, dim3(g), dim3(64), 0, 0, (const double *)ws, (double *)io.dout, n);
        }
        io.finish("epnp_split");
        HIP_OK(hipFree(ws));
    }
    if (load("fast_pair", 4, in) && in.size() == 4) {
        int max_tuples;
        memcpy(&max_tuples, in.data(), 4);
        if (max_tuples < 0 || max_tuples > 4096)
            fail("fast_pair", "max_tuples out of range");
        std::vector<int> centres; // the centres of ke_fast_compass_pair_check
        for (int v0 = 0; v0 < 256; v0 += (v0 < 24 || v0 > 230 ? 1 : 5))
            centres.push_back(v0);
        std::vector<char> cin(centres.size() * 4);
        memcpy(cin.data(), centres.data(), cin.size());
        DevIo io(cin, 16 + (size_t)max_tuples * 32);
        unsigned long long *res = nullptr; // disagreements, comparisons, tuple slots handed out
        HIP_OK(hipMalloc((void **)&res, 24));
        HIP_OK(hipMemset(res, 0, 24));
        hipLaunchKernelGGL(fast_pair_kernel, dim3((unsigned)centres.size(), 8), dim3(256), 0, 0, (const int *)io.din, res,
                           (uint32_t *)(io.dout + 16), max_tuples);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(io.dout, res, 16, hipMemcpyDeviceToDevice));
        io.finish("fast_pair");
        HIP_OK(hipFree(res));
    }
}

int main(int argc, char **argv)
{
    bool host = false;
    int a = 1;
    if (a < argc && strcmp(argv[a], "--host") == 0) {
        host = true;
        a++;
    }
    if (a + 1 != argc) {
        printf("FAIL: usage: device_check [--host] <dir>\n");
        return 2;
    }
    g_dir = argv[a];
    if (!host) {
        int count = 0;
        HIP_OK(hipGetDeviceCount(&count));
        if (count < 1)
            fail("hipGetDeviceCount", "no device");
        HIP_OK(hipSetDevice(0));
    }
    run_cases(uc::AllOps(), host);
    if (!host)
        run_wide();
    printf("OK%s\n", g_done.c_str());
    return 0;
}
