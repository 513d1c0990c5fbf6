// cbet_mix.hip -- the Anderson mixing of the gain iterate on the device (no reference counterpart):
//   * k_mix_residual<H> : f = y - x and the H + 1 dot products of f with the H held residuals and itself, one partial row per
//                         workgroup
//   * k_mix_reduce      : the partial rows, in index order, into the caller's row
//   * k_mix_apply<C>    : x = sum_j alpha_j y_j over C held iterates, oldest first, to x_out and (if asked) x_keep
// and their C entries (the refusals are the host twins', cbet_mix_host.cpp).  The statements and the order of every sum are
// cbet_mix_model.h's; built with -ffp-contract=off like the rest of the library, so the kernels agree with the twins bit for bit.
// Streaming kernels over plain arrays: a thread owns PAIRS of consecutive elements (written as two 8-byte accesses, which is all
// the alignment of a double promises; the compiler merges them into one 16-byte access, which global memory takes at any
// 8-byte boundary -- global_load / global_store_dwordx4 in the listing -- and which changes no sum), takes all pairs of a span
// into registers before it stores any (kMixIters independent loads per array in flight), and the spans go round-robin to at
// most CBET_MIX_MAX_GROUPS workgroups.  Their own translation unit: no other kernel sees a changed line.
#include <hip/hip_runtime.h>

#include "cbet_device.h"
#include "cbet_host_internal.h"
#include "cbet_mix_model.h"

namespace cbet {
namespace {

static_assert(kMixWave == kWave, "the model's wavefront is the device's");

struct MixResidualArgs {
    const double *y, *x;
    double *f;
    const double *fh[CBET_MIX_MAX_DEPTH];
    long n;
};
struct MixApplyArgs {
    const double *y[CBET_MIX_MAX_DEPTH + 1];       // no restrict anywhere: x_out may be one of them
    double alpha[CBET_MIX_MAX_DEPTH + 1];
    double *x_out, *x_keep;
    long n;
};

__device__ __forceinline__ void load_pair(const double *p, long e, double &a, double &b) { a = p[e]; b = p[e + 1]; }
__device__ __forceinline__ void store_pair(double *p, long e, double a, double b) { p[e] = a; p[e + 1] = b; }

// The wavefront's sum in every lane: six butterfly steps (the adds commute, so both lanes of a pair hold the same bits).
__device__ __forceinline__ double wave_sum(double s)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) s = s + __shfl_xor(s, off, kWave);
    return s;
}
// NV thread sums per thread -> the workgroup's, in thread 0: the wavefronts in order.  part: [kMixThreads / kWave][NV] in LDS.
template <int NV>
__device__ __forceinline__ void workgroup_sum(double (&v)[NV], double (*part)[NV])
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const double s = wave_sum(v[j]);
        if (lane == 0) part[wave][j] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            double t = part[0][j];
            for (int w = 1; w < kMixThreads / kWave; ++w) t = t + part[w][j];
            v[j] = t;
        }
    }
}

template <int H>
__global__ void __launch_bounds__(kMixThreads) k_mix_residual(const MixResidualArgs a, double *__restrict__ work)
{
    const int t = threadIdx.x;
    const long spans = mix_spans(a.n);
    double dot[H + 1];
#pragma unroll
    for (int j = 0; j <= H; ++j) dot[j] = 0.0;
    for (long s = blockIdx.x; s < spans; s += gridDim.x) {
        if ((s + 1) * CBET_MIX_SPAN <= a.n) {              // a whole span: every pair into registers, then the arithmetic and the stores
            double y[kMixIters][2], x[kMixIters][2], fh[kMixIters][2][H > 0 ? H : 1];
#pragma unroll
            for (int i = 0; i < kMixIters; ++i) {
                const long e = mix_element(s, i, t);
                load_pair(a.y, e, y[i][0], y[i][1]);
                load_pair(a.x, e, x[i][0], x[i][1]);
#pragma unroll
                for (int j = 0; j < H; ++j) load_pair(a.fh[j], e, fh[i][0][j], fh[i][1][j]);
            }
#pragma unroll
            for (int i = 0; i < kMixIters; ++i) {
                const double f0 = mix_residual_element<H>(y[i][0], x[i][0], fh[i][0], dot);
                const double f1 = mix_residual_element<H>(y[i][1], x[i][1], fh[i][1], dot);
                store_pair(a.f, mix_element(s, i, t), f0, f1);
            }
        } else {                                           // the ragged last span: element by element, the same order
#pragma unroll
            for (int i = 0; i < kMixIters; ++i)
                for (long e = mix_element(s, i, t), last = e + 1; e <= last && e < a.n; ++e) {
                    double fh[H > 0 ? H : 1];
#pragma unroll
                    for (int j = 0; j < H; ++j) fh[j] = a.fh[j][e];
                    a.f[e] = mix_residual_element<H>(a.y[e], a.x[e], fh, dot);
                }
        }
    }
    __shared__ double part[kMixThreads / kWave][H + 1];
    workgroup_sum<H + 1>(dot, part);
    if (t == 0) {
#pragma unroll
        for (int j = 0; j <= H; ++j) work[(long)blockIdx.x * kMixRow + j] = dot[j];
    }
}

// One workgroup: thread t sums the partial rows t, t + 256, ... in that order, then the workgroup's order again.
__global__ void __launch_bounds__(kMixThreads) k_mix_reduce(const double *__restrict__ work, int groups, int nv, double *__restrict__ row)
{
    double s[kMixRow];
#pragma unroll
    for (int j = 0; j < kMixRow; ++j) s[j] = 0.0;
    for (int g = threadIdx.x; g < groups; g += kMixThreads) {
#pragma unroll
        for (int j = 0; j < kMixRow; ++j)
            if (j < nv) s[j] = s[j] + work[(long)g * kMixRow + j];
    }
    __shared__ double part[kMixThreads / kWave][kMixRow];
    workgroup_sum<kMixRow>(s, part);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < kMixRow; ++j)
            if (j < nv) row[j] = s[j];
    }
}

template <int C>
__global__ void __launch_bounds__(kMixThreads) k_mix_apply(const MixApplyArgs a)
{
    const int t = threadIdx.x;
    const long spans = mix_spans(a.n);
    for (long s = blockIdx.x; s < spans; s += gridDim.x) {
        if ((s + 1) * CBET_MIX_SPAN <= a.n) {
            double y[kMixIters][2][C];
#pragma unroll
            for (int i = 0; i < kMixIters; ++i) {
                const long e = mix_element(s, i, t);
#pragma unroll
                for (int j = 0; j < C; ++j) load_pair(a.y[j], e, y[i][0][j], y[i][1][j]);
            }
#pragma unroll
            for (int i = 0; i < kMixIters; ++i) {          // this thread's elements are read: x_out may now overwrite one of the y
                const long e = mix_element(s, i, t);
                const double v0 = mix_combine<C>(y[i][0], a.alpha), v1 = mix_combine<C>(y[i][1], a.alpha);
                store_pair(a.x_out, e, v0, v1);
                if (a.x_keep) store_pair(a.x_keep, e, v0, v1);
            }
        } else {
#pragma unroll
            for (int i = 0; i < kMixIters; ++i)
                for (long e = mix_element(s, i, t), last = e + 1; e <= last && e < a.n; ++e) {
                    double y[C];
#pragma unroll
                    for (int j = 0; j < C; ++j) y[j] = a.y[j][e];
                    const double v = mix_combine<C>(y, a.alpha);
                    a.x_out[e] = v;
                    if (a.x_keep) a.x_keep[e] = v;
                }
        }
    }
}

template <int H>
void launch_residual(const MixResidualArgs &a, long groups, double *work, hipStream_t stream)
{
    hipLaunchKernelGGL(k_mix_residual<H>, dim3((unsigned)groups), dim3(kMixThreads), 0, stream, a, work);
}
template <int C>
void launch_apply(const MixApplyArgs &a, long groups, hipStream_t stream)
{
    hipLaunchKernelGGL(k_mix_apply<C>, dim3((unsigned)groups), dim3(kMixThreads), 0, stream, a);
}

}  // namespace
}  // namespace cbet

extern "C" int cbet_mix_residual(const double *y, const double *x, double *f, const double *const *f_held, int h, long n,
                                 double *row, void *work, void *stream)
{
    using namespace cbet;
    if (int rc = mix_residual_check("cbet_mix_residual", y, x, f, f_held, h, n, row)) return rc;
    if (n > 0 && !work) return fail(CBET_EINVAL, "cbet_mix_residual: work is NULL (cbet_mix_work_bytes)");
    MixResidualArgs a{};
    a.y = y; a.x = x; a.f = f; a.n = n;
    for (int j = 0; j < h; ++j) a.fh[j] = f_held[j];
    const long groups = mix_groups(n);
    if (groups > 0) {
        switch (h) {
        case 0: launch_residual<0>(a, groups, (double *)work, (hipStream_t)stream); break;
        case 1: launch_residual<1>(a, groups, (double *)work, (hipStream_t)stream); break;
        case 2: launch_residual<2>(a, groups, (double *)work, (hipStream_t)stream); break;
        case 3: launch_residual<3>(a, groups, (double *)work, (hipStream_t)stream); break;
        default: launch_residual<4>(a, groups, (double *)work, (hipStream_t)stream); break;
        }
        CBET_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_mix_reduce, dim3(1), dim3(kMixThreads), 0, (hipStream_t)stream, (const double *)work, (int)groups, h + 1, row);
    CBET_HIP(hipGetLastError());
    return CBET_OK;
}

extern "C" int cbet_mix_apply(const double *const *y_held, const double *alpha, int count, long n, double *x_out, double *x_keep,
                              void *stream)
{
    using namespace cbet;
    if (int rc = mix_apply_check("cbet_mix_apply", y_held, alpha, count, n, x_out)) return rc;
    MixApplyArgs a{};
    a.x_out = x_out; a.x_keep = x_keep; a.n = n;
    for (int j = 0; j < count; ++j) { a.y[j] = y_held[j]; a.alpha[j] = alpha[j]; }
    const long groups = mix_groups(n);
    if (groups == 0) return CBET_OK;
    switch (count) {
    case 1: launch_apply<1>(a, groups, (hipStream_t)stream); break;
    case 2: launch_apply<2>(a, groups, (hipStream_t)stream); break;
    case 3: launch_apply<3>(a, groups, (hipStream_t)stream); break;
    case 4: launch_apply<4>(a, groups, (hipStream_t)stream); break;
    default: launch_apply<5>(a, groups, (hipStream_t)stream); break;
    }
    CBET_HIP(hipGetLastError());
    return CBET_OK;
}
