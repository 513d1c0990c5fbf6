// cbet_trace_exit.hip -- the trajectory-only exit pass for gfx950 (CDNA4) and the two reductions of its records
// (DESIGN.md section 10).
//
//   * k_trace_exit<GAIN, IDX64> : traces the rays of a deposit pass and deposits nothing.  One wavefront = one bundle
//     of the context's launch list (work_item / launch_ray of cbet_trace_common.h, the shipped kernel's beam range,
//     shard split and grid_beam0).  A ray's position, velocity, cell, energy and step count are the reference's
//     arithmetic, operation for operation (/root/reference/launch_ray_XZ.cu:207-357, built with -ffp-contract=off):
//     kick from the step record of its node, drift, nearest-node update (cbet_relocate.h relocate_closed), absorption,
//     the stop test of :351-356.  When the ray ends -- in the step where that test first holds, or after nt steps --
//     its lane writes one cbet_ray_exit record.  GAIN: the CBET hook of k_trace_window<16, ., 1> (cbet_trace_window.hip,
//     the `if (gk)` block) before the absorption, so that a ray's exit energy is what the CBET deposition pass leaves it.
//   * k_exit_tally  : per-beam energy balance of the records, one workgroup per beam, fixed summation order (no atomics:
//     bit-reproducible from run to run).
//   * k_farfield    : the escaped rays' energy binned by exit direction (equal solid angle per polar bin), ADDED into a
//     histogram with fp64 atomics.
//
// Nothing here is hand-scheduled: the step record is an ordinary load whose wait the compiler places.
#include <hip/hip_runtime.h>

#include "cbet_trace_common.h"

namespace cbet {

static_assert(sizeof(cbet_ray_exit) == 80, "cbet_ray_exit is 80 bytes (include/cbet_mi355x.h)");
static_assert(sizeof(cbet_ray_exit) == kExitDoubles * sizeof(double), "kExitDoubles doubles per record");

namespace {

// The step record (cbet_device.h StepRecord) of node `cell`: a 32-byte gather.  IDX64 = false: the table is at most
// 2^32 bytes, so the byte offset is a 32-bit one (scalar base + vector offset).
template <bool IDX64>
__device__ __forceinline__ StepRecord load_record(const TraceArgs &a, unsigned cell)
{
#ifdef CBET_DEBUG_BOUNDS
    if (!(cell < a.audit_nodes)) { audit_fail(a); return StepRecord{0.0, 0.0, 0.0, 0.0}; }
#endif
    if (IDX64) return a.steprec[cell];
    return *reinterpret_cast<const StepRecord *>(reinterpret_cast<const char *>(a.steprec) + (cell << 5));
}

// An axis's two deposit factors in the shipped kernel's lane-dependent order (cbet_trace_window.hip, `pair`): F0 = |o|
// for an unflipped lane, 1 - |o| for a flipped one; F1 = 1 - F0.  The gain sum below then rounds exactly as the
// shipped CBET kernel's does for the same lane.
__device__ __forceinline__ void factor_pair(double o, int flip, double &f0, double &f1)
{
    const double g = fabs(o) - (double)flip;
    f0 = __hiloint2double(__double2hiint(g) ^ (flip << 31), __double2loint(g));
    f1 = 1.0 - f0;
}

template <bool GAIN, bool IDX64>
__global__ void __launch_bounds__(kWave) k_trace_exit(const TraceArgs a)
{
    const int lane = threadIdx.x;
    int beam, patch;
    if (!work_item(a, blockIdx.x, beam, patch)) return;   // wave-uniform

    const int li = patch * kWave + lane;
    const bool has_slot = li < a.nlive;                   // the list is whole bundles; this is a guard only
    const int pre_raynum = has_slot ? a.live[li] : -1;   // -1: idle lane of the bundle
    Ray s = {};
    bool launched = pre_raynum >= 0;
    if (launched) launched = launch_ray(a, beam, pre_raynum, s);
    const double uray0 = s.uray;                          // :113

    const int nx = a.nx, ny = a.ny, nz = a.nz;
    const double xlo = a.bounds[0], xhi = a.bounds[1], ylo = a.bounds[2], yhi = a.bounds[3], zlo = a.bounds[4],
                 zhi = a.bounds[5];
    StepRecord rec = {0.0, 0.0, 0.0, 0.0};
    if (launched) rec = load_record<IDX64>(a, (unsigned)((s.ci * ny + s.cj) * nz + s.ck));   // :254-270 at the launch node

    const double *const gk = GAIN ? a.gain + (long)(beam - a.grid_beam0) * a.hsize : nullptr;
    const int sYh = a.sYh, sXh = a.sXh;
    // the shipped kernel's lane flips (cbet_trace_window.hip): which of an axis's two nodes the lane takes first
    const int pfx = lane & 1, pfy = (lane >> 1) & 1, pfz = (lane >> 3) & 1;
    double gained = 0.0;

    bool alive = launched;
    int steps = 0, status = 0;
    for (int tt = 0; tt < a.nt; ++tt) {                   // :207
        if (__builtin_amdgcn_ballot_w64(alive) == 0ull) break;
        double x = 0.0;                                   // GAIN: the clamped exponent K ds of the step
        if (alive) {
            // :268-273 kick, drift
            s.vx -= rec.kx;
            s.vy -= rec.ky;
            s.vz -= rec.kz;
            s.px += s.vx * a.dt;
            s.py += s.vy * a.dt;
            s.pz += s.vz * a.dt;
            // :276-292 position in cell units, nearest-node update
            const double fx = (s.px - a.xmin) * a.inv_dx;
            const double fy = (s.py - a.ymin) * a.inv_dy;
            const double fz = (s.pz - a.zmin) * a.inv_dz;
            s.ci = relocate_closed(s.ci, fx, nx);
            s.cj = relocate_closed(s.cj, fy, ny);
            s.ck = relocate_closed(s.ck, fz, nz);
            // :296-305 the absorption coefficient now, the kicks of the next step
            rec = load_record<IDX64>(a, (unsigned)((s.ci * ny + s.cj) * nz + s.ck));
            if (GAIN) {
                // K at the eight deposit nodes with the deposit weights (:319-339), as k_trace_window<16, ., 1> gathers it
                const double ox = (fx - (double)s.ci) - 0.5, oy = (fy - (double)s.cj) - 0.5, oz = (fz - (double)s.ck) - 0.5;
                const bool ngx = ox < 0, ngy = oy < 0, ngz = oz < 0;
                const int lx = s.ci + 1 - (ngx ? 1 : 0), ly = s.cj + 1 - (ngy ? 1 : 0), lz = s.ck + 1 - (ngz ? 1 : 0);
                const bool hx = ngx != (pfx != 0), hy = ngy != (pfy != 0), hz = ngz != (pfz != 0);
                const int X0 = lx + (hx ? 1 : 0), X1 = lx + (hx ? 0 : 1);
                const int Y0 = ly + (hy ? 1 : 0), Y1 = ly + (hy ? 0 : 1);
                const int Z0 = lz + (hz ? 1 : 0), Z1 = lz + (hz ? 0 : 1);
                double Fx0, Fx1, Fy0, Fy1, Fz0, Fz1;
                factor_pair(ox, pfx, Fx0, Fx1);
                factor_pair(oy, pfy, Fy0, Fy1);
                factor_pair(oz, pfz, Fz0, Fz1);
                const double ds = sqrt_speed(__builtin_fma(s.vz, s.vz, __builtin_fma(s.vy, s.vy, s.vx * s.vx))) * a.dt;
                const int nX0 = X0 * sXh, nX1 = X1 * sXh, nY0 = Y0 * sYh, nY1 = Y1 * sYh;
                const bool z0_low = Z0 < Z1;
                const int zl = z0_low ? Z0 : Z1;
                const double fz_lo = z0_low ? Fz0 : Fz1, fz_hi = z0_low ? Fz1 : Fz0;
                const gain_pair_t c00 = gain_load2<IDX64>(a, gk, (unsigned)(nX0 + nY0 + zl)), c10 = gain_load2<IDX64>(a, gk, (unsigned)(nX1 + nY0 + zl));
                const gain_pair_t c01 = gain_load2<IDX64>(a, gk, (unsigned)(nX0 + nY1 + zl)), c11 = gain_load2<IDX64>(a, gk, (unsigned)(nX1 + nY1 + zl));
                const double q00 = __builtin_fma(fz_hi, c00.y, fz_lo * c00.x), q10 = __builtin_fma(fz_hi, c10.y, fz_lo * c10.x);
                const double q01 = __builtin_fma(fz_hi, c01.y, fz_lo * c01.x), q11 = __builtin_fma(fz_hi, c11.y, fz_lo * c11.x);
                const double r0 = __builtin_fma(Fx1, q10, Fx0 * q00), r1 = __builtin_fma(Fx1, q11, Fx0 * q01);
                const double ksum = __builtin_fma(Fy1, r1, Fy0 * r0);
                x = ksum * ds;
                if (x > a.max_exponent) x = a.max_exponent;
                if (x < -a.max_exponent) x = -a.max_exponent;
            }
        }
        if (GAIN) {
            // the shipped kernel's wave-wide choice of the series: the short one when every live lane's |x| is small
            const bool small = __builtin_amdgcn_ballot_w64(alive && !(fabs(x) < 0.03125)) == 0ull;
            if (alive) {
                const double phi = small ? phi_small(x) : phi_det(x);
                const double dg = s.uray * (x * phi);
                gained += dg;
                s.uray = s.uray + dg;
            }
        }
        if (alive) {
            s.uray -= rec.kap * s.uray;                   // :305-311 (absorbing mode only: checked on the host)
            // :351-356 the stop test; the record says which of its conditions held
            const bool cut = s.uray <= s.ustop;
            const bool out = s.px < xlo || s.px > xhi || s.py < ylo || s.py > yhi || s.pz < zlo || s.pz > zhi;
            if (cut || out) {
                alive = false;
                steps = tt + 1;
                status = CBET_RAY_LAUNCHED | (cut ? CBET_RAY_CUTOFF : 0) | (out ? CBET_RAY_ESCAPED : 0);
            }
        }
    }
    if (alive) {                                          // ran out of steps (:207)
        steps = a.nt;
        status = CBET_RAY_LAUNCHED | CBET_RAY_TIMEOUT;
    }

    if (has_slot) {
        cbet_ray_exit e = {};
        if (launched) {
            e.x = s.px; e.y = s.py; e.z = s.pz;
            e.vx = s.vx; e.vy = s.vy; e.vz = s.vz;
            e.uray = s.uray; e.uray0 = uray0; e.gained = gained;
            e.steps = steps; e.status = status;
        }
        // records of beam b: [(b - grid_beam0) * L, ... + L), L = the launch list's length (edep / grid_stride, see
        // launch_trace_exit)
        cbet_ray_exit *const dst = reinterpret_cast<cbet_ray_exit *>(a.edep + (long)(beam - a.grid_beam0) * a.grid_stride) + li;
#ifdef CBET_DEBUG_BOUNDS
        const double *lo = reinterpret_cast<const double *>(dst);
        if (!(lo >= a.audit_lo && lo + kExitDoubles <= a.audit_hi)) audit_fail(a);
        else
#endif
        *dst = e;
    }

    const int tot_steps = wave_sum(launched ? steps : 0), tot_rays = wave_sum(launched ? 1 : 0);
    if (lane == 0) {
        atomicAdd(&a.counters[kCntSteps], (unsigned long long)tot_steps);
        atomicAdd(&a.counters[kCntRays], (unsigned long long)tot_rays);
    }
}

// ---------------------------------------------------------------------------------------------
// Energy balance: workgroup b sums the L records of beam b.  Thread t takes records t, t + 256, ... in that order, then
// a fixed pairwise tree in LDS: the same sums in the same order on every run.
// ---------------------------------------------------------------------------------------------
constexpr int kTallyThreads = 256;

__global__ void __launch_bounds__(kTallyThreads) k_exit_tally(const cbet_ray_exit *exits, long L, double *tally)
{
    __shared__ double red[CBET_TALLY_COLUMNS][kTallyThreads];
    const int t = threadIdx.x;
    const cbet_ray_exit *const e = exits + (long)blockIdx.x * L;
    double acc[CBET_TALLY_COLUMNS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long i = t; i < L; i += kTallyThreads) {
        const cbet_ray_exit r = e[i];
        if (!(r.status & CBET_RAY_LAUNCHED)) continue;
        acc[0] += r.uray0;                               // launched
        acc[1] += r.gained;                              // gained
        acc[2] += (r.uray0 + r.gained) - r.uray;         // absorbed
        if (r.status & CBET_RAY_ESCAPED) acc[3] += r.uray;        // escaped
        else if (r.status & CBET_RAY_CUTOFF) acc[4] += r.uray;    // stranded
        else acc[5] += r.uray;                                    // unfinished
        acc[6] += 1.0;                                   // n_rays
        if (r.status & CBET_RAY_ESCAPED) acc[7] += 1.0;  // n_escaped
    }
#pragma unroll
    for (int c = 0; c < CBET_TALLY_COLUMNS; ++c) red[c][t] = acc[c];
    __syncthreads();
    for (int half = kTallyThreads / 2; half > 0; half >>= 1) {
        if (t < half) {
#pragma unroll
            for (int c = 0; c < CBET_TALLY_COLUMNS; ++c) red[c][t] += red[c][t + half];
        }
        __syncthreads();
    }
    if (t < CBET_TALLY_COLUMNS) tally[(long)blockIdx.x * CBET_TALLY_COLUMNS + t] = red[t][0];
}

// ---------------------------------------------------------------------------------------------
// Far field: an escaped ray's remaining energy goes to the bin of its exit direction v / |v|:
//   it = min(ntheta - 1, floor((1 - vz / |v|) / 2 * ntheta))      (equal solid angle per polar bin)
//   ip = min(nphi - 1, floor((atan2(vy, vx) + pi) / (2 pi) * nphi))
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int bin_of(double c, int n)
{
    if (!(c > 0.0)) return 0;                            // (NaN too: a ray without a direction)
    const double f = floor(c);
    return f >= (double)(n - 1) ? n - 1 : (int)f;
}

__global__ void __launch_bounds__(256) k_farfield(const cbet_ray_exit *exits, long n, int ntheta, int nphi, double *hist)
{
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const cbet_ray_exit r = exits[i];
        if ((r.status & (CBET_RAY_LAUNCHED | CBET_RAY_ESCAPED)) != (CBET_RAY_LAUNCHED | CBET_RAY_ESCAPED)) continue;
        const double vn = sqrt(r.vx * r.vx + r.vy * r.vy + r.vz * r.vz);
        const int it = bin_of((1.0 - r.vz / vn) / 2.0 * ntheta, ntheta);
        const int ip = bin_of((atan2(r.vy, r.vx) + M_PI) / (2.0 * M_PI) * nphi, nphi);
        unsafeAtomicAdd(&hist[(long)it * nphi + ip], r.uray);
    }
}

}  // namespace

// `a` is a trace's argument block with the records in place of the deposit grid: edep = the record array as doubles,
// grid_stride = kExitDoubles * L doubles per beam (so the audited range of launch_trace covers exactly the records the
// launch's beams may write).
hipError_t launch_trace_exit(const TraceArgs &a, bool force_idx64, hipStream_t stream)
{
    const long waves = a.item_count;
    if (waves <= 0) return hipSuccess;
    const dim3 grid((unsigned)waves), block(kWave);
    const bool wide = force_idx64 || sizeof(StepRecord) * (unsigned long long)a.nx * a.ny * a.nz > (1ull << 32) ||
                      (a.gain && 8ull * (unsigned long long)a.hsize >= (1ull << 32));
    if (a.gain) {
        if (wide) hipLaunchKernelGGL((k_trace_exit<true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((k_trace_exit<true, false>), grid, block, 0, stream, a);
    } else {
        if (wide) hipLaunchKernelGGL((k_trace_exit<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((k_trace_exit<false, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_exit_tally(const cbet_ray_exit *exits, long L, int nbeams, double *tally, hipStream_t stream)
{
    if (nbeams <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_exit_tally, dim3((unsigned)nbeams), dim3(kTallyThreads), 0, stream, exits, L, tally);
    return hipGetLastError();
}

hipError_t launch_farfield(const cbet_ray_exit *exits, long n, int ntheta, int nphi, double *hist, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    long blocks = (n + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(k_farfield, dim3((unsigned)blocks), dim3(256), 0, stream, exits, n, ntheta, nphi, hist);
    return hipGetLastError();
}

}  // namespace cbet
