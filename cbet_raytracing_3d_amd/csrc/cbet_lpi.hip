// cbet_lpi.hip -- the quarter-critical LPI maps on the device (no reference counterpart, parity unpinned):
//   * k_lpi_map    : normalised fields + the node density table -> lpi[CBET_LPI_NQ][hsize] over the planes [hx_lo, hx_hi), and
//                    one partial cbet_lpi_summary per workgroup
//   * k_lpi_reduce : the partial summaries, in workgroup order, merged into the caller's summary
// The model -- band, gradient, scale length, presence, cone bin, threshold parameter, the summary's merge -- is
// cbet_lpi_model.h's, written once for k_lpi_map and the host twin (cbet_lpi_host.cpp).  Built with -ffp-contract=off like the
// rest of the library: every statement is one IEEE operation in the order written, so the map agrees with the twin bit for bit.
// Its own translation unit and its own argument block (LpiArgs): no kernel of the gain stage sees a changed line.
#include <hip/hip_runtime.h>

#include "cbet_device.h"
#include "cbet_host_internal.h"
#include "cbet_lpi_model.h"

namespace cbet {
namespace {

// The walk of the gain stage's k_gain_field and k_pair_amplitude (cbet_grid_kernels.hip brick_cell), on this block: one
// wavefront per 2 x 4 x 8 brick of deposit-grid cells, z fastest (every access is eight 64-byte runs), the bricks that touch
// the slab [hx_lo, hx_hi) in z, y, x order.  h: the lane's cell of the haloed grid, 0 where the lane has none.
struct LpiBrickCell { bool valid; long h; };
__device__ __forceinline__ long lpi_brick_count(const LpiArgs &a) { return (long)(((a.hx_hi + 1) >> 1) - (a.hx_lo >> 1)) * ((a.ny + 5) / 4) * ((a.nz + 9) / 8); }
__device__ __forceinline__ LpiBrickCell lpi_brick_cell(const LpiArgs &a, long brick, int lane)
{
    const int HY = a.ny + 2, HZ = a.nz + 2;
    const int bx0 = a.hx_lo >> 1, by = (HY + 3) / 4, bz = (HZ + 7) / 8;
    const int ibz = (int)(brick % bz);
    const long t = brick / bz;
    const int iby = (int)(t % by), ibx = bx0 + (int)(t / by);
    const int hi = 2 * ibx + (lane >> 5), hj = 4 * iby + ((lane >> 3) & 3), hk = 8 * ibz + (lane & 7);
    const bool valid = hi >= a.hx_lo && hi < a.hx_hi && hj < HY && hk < HZ;
    return {valid, valid ? ((long)hi * HY + hj) * HZ + hk : 0L};
}

// The summary of lane (lane ^ off): twelve shuffles.  Both lanes of a pair then merge the other's into their own -- the
// adds commute, so the pair holds the same bits, and after six steps every lane holds the wavefront's summary.
__device__ __forceinline__ cbet_lpi_summary summary_of_lane_xor(const cbet_lpi_summary &s, int off)
{
    cbet_lpi_summary t;
    t.band_cells = __shfl_xor(s.band_cells, off, kWave);
    t.lit_cells = __shfl_xor(s.lit_cells, off, kWave);
    t.above_max = __shfl_xor(s.above_max, off, kWave);
    t.above_cw = __shfl_xor(s.above_cw, off, kWave);
    t.above_sum = __shfl_xor(s.above_sum, off, kWave);
    t.argmax_cw = __shfl_xor(s.argmax_cw, off, kWave);
    t.max_eta_max = __shfl_xor(s.max_eta_max, off, kWave);
    t.max_eta_cw = __shfl_xor(s.max_eta_cw, off, kWave);
    t.max_eta_sum = __shfl_xor(s.max_eta_sum, off, kWave);
    t.sum_I_sum = __shfl_xor(s.sum_I_sum, off, kWave);
    t.sum_I_cw = __shfl_xor(s.sum_I_cw, off, kWave);
    t.max_present = __shfl_xor(s.max_present, off, kWave);
    t.reserved = 0;
    return t;
}
__device__ __forceinline__ void wave_merge(cbet_lpi_summary &s)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const cbet_lpi_summary t = summary_of_lane_xor(s, off);
        lpi_summary_merge(s, t);
    }
}

// fields (I, kx, ky, kz) + ne3d -> the seven quantities of every cell of the slab, brick by brick.
//   band first: a wavefront whose ballot of in-band lanes is empty writes its zeros and never touches `fields` -- at 256^3 the
//            default band holds well under 1 % of the cells, and the kernel is then ne3d in, zeros out.  The six neighbours of
//            the gradient are read by in-band lanes only.
//   beams  : the set of beams with I > 0 in some in-band cell of the brick (a ballot-built bit mask, as k_gain_field's), in
//            increasing order; a lane loads a beam's direction only where its own I > 0.
//   bins   : CAP >= NB bin sums per lane in registers, updated by an unrolled select chain (never indexed by the run-time
//            bin: no private array, no scratch).  Bins NB .. CAP-1 stay 0 and never win the maximum.  CAP = 1 (NB = 1): the
//            only bin's sum is I_sum's own chain of adds, the same bits.
//   summary: every lane merges its band cells in brick order (lpi_summary_cell), the wavefront merges its lanes by six
//            butterfly steps, the workgroup's first thread merges the four wavefronts in order and stores work[blockIdx.x].
template <int CAP>
__global__ void __launch_bounds__(256) k_lpi_map(const LpiArgs a, cbet_lpi_summary *__restrict__ work)
{
    const long total = a.hsize * a.nbeams;
    const long bricks = lpi_brick_count(a);
    const int lane = threadIdx.x & (kWave - 1);
    const long wave0 = (long)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
    const long nwaves = (long)gridDim.x * (blockDim.x / kWave);
    cbet_lpi_summary s;
    lpi_summary_clear(s);
    for (long brick = wave0; brick < bricks; brick += nwaves) {
        const LpiBrickCell cell = lpi_brick_cell(a, brick, lane);
        int i, j, k;
        lpi_cell_node(a, cell.h, i, j, k);
        const double ne = a.ne3d[((long)i * a.ny + j) * a.nz + k];
        const bool band = cell.valid && lpi_in_band(a, ne / a.ncrit);
        LpiCell c = {0.0, 0.0, 0.0, 0};
        LpiPlasma q = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (__builtin_amdgcn_ballot_w64(band) != 0ull) {
            if (band) q = lpi_plasma(a, i, j, k, ne);
            const double *fI = a.fields + cell.h, *fx = fI + total, *fy = fx + total, *fz = fy + total;
            unsigned long long mask = 0ull;             // beams with I > 0 in some in-band cell of this brick
            for (int b = 0; b < a.nbeams; ++b) {
                const double I = band ? fI[(long)b * a.hsize] : 0.0;
                if (__builtin_amdgcn_ballot_w64(I > 0.0) != 0ull) mask |= 1ull << b;
            }
            double bins[CAP];
#pragma unroll
            for (int n = 0; n < CAP; ++n) bins[n] = 0.0;
            while (mask != 0ull) {
                const int b = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const long o = (long)b * a.hsize;
                const double I = band ? fI[o] : 0.0;
                if (I > 0.0) {
                    const double kx = fx[o], ky = fy[o], kz = fz[o], kn = lpi_knorm(kx, ky, kz);
                    if (lpi_present(I, kn)) {
                        c.Isum = c.Isum + I;
                        if (I > c.Imax) c.Imax = I;
                        c.npresent += 1;
                        if constexpr (CAP > 1) {
                            const int bin = lpi_bin(q, kx, ky, kz, kn, a.cone_bins);
#pragma unroll
                            for (int n = 0; n < CAP; ++n) bins[n] = n == bin ? bins[n] + I : bins[n];
                        }
                    }
                }
            }
            if constexpr (CAP > 1) {
#pragma unroll
                for (int n = 0; n < CAP; ++n)
                    if (bins[n] > c.Icw) c.Icw = bins[n];
            } else {
                c.Icw = c.Isum;
            }
            if (band) lpi_summary_cell(s, cell.h, c, q);
        }
        if (cell.valid) lpi_store(a, cell.h, band, c, q);
    }
    if (!work) return;
    __shared__ cbet_lpi_summary part[256 / kWave];
    wave_merge(s);
    if (lane == 0) part[threadIdx.x / kWave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        cbet_lpi_summary t = part[0];
        for (int w = 1; w < 256 / kWave; ++w) lpi_summary_merge(t, part[w]);
        work[blockIdx.x] = t;
    }
}

// One wavefront: lane l merges partials l, l + 64, ... in that order, six butterfly steps merge the lanes, lane 0 merges the
// result into the caller's summary.  A fixed order for a given number of workgroups: two calls give the same bits.
__global__ void __launch_bounds__(64) k_lpi_reduce(const cbet_lpi_summary *__restrict__ work, int groups, cbet_lpi_summary *__restrict__ out)
{
    cbet_lpi_summary s;
    lpi_summary_clear(s);
    for (int g = threadIdx.x; g < groups; g += kWave) lpi_summary_merge(s, work[g]);
    wave_merge(s);
    if (threadIdx.x == 0) {
        cbet_lpi_summary t = *out;
        lpi_summary_merge(t, s);
        *out = t;
    }
}

}  // namespace

hipError_t launch_lpi_map(const LpiArgs &a, cbet_lpi_summary *summary, cbet_lpi_summary *work, long groups, hipStream_t stream)
{
    if (a.hx_hi <= a.hx_lo || groups <= 0) return hipSuccess;
    cbet_lpi_summary *partials = summary ? work : nullptr;
    const dim3 grid((unsigned)groups), block(256);
    if (a.cone_bins == 1) hipLaunchKernelGGL(k_lpi_map<1>, grid, block, 0, stream, a, partials);
    else if (a.cone_bins <= 8) hipLaunchKernelGGL(k_lpi_map<8>, grid, block, 0, stream, a, partials);
    else hipLaunchKernelGGL(k_lpi_map<CBET_LPI_MAX_BINS>, grid, block, 0, stream, a, partials);
    if (hipError_t e = hipGetLastError()) return e;
    if (!summary) return hipSuccess;
    hipLaunchKernelGGL(k_lpi_reduce, dim3(1), dim3(kWave), 0, stream, partials, (int)groups, summary);
    return hipGetLastError();
}

}  // namespace cbet
