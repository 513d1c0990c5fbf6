// cbet_trace_exit.hip -- the trajectory-only exit pass for gfx950 (CDNA4) and the two reductions of its records
// (DESIGN.md section 10).
//
//   * k_trace_exit<GAIN, IDX64> : traces the rays of a deposit pass and deposits nothing.  One wavefront = one bundle
//     of the context's launch list (work_item / launch_ray of cbet_trace_common.h, the shipped kernel's beam range,
//     shard split and grid_beam0).  A ray's position, velocity, cell, energy and step count are the reference's
//     arithmetic, operation for operation (/root/reference/launch_ray_XZ.cu:207-357, built with -ffp-contract=off):
//     kick from the step record of its node, drift, nearest-node update (cbet_relocate.h relocate_closed), absorption,
//     the stop test of :351-356.  When the ray ends -- in the step where that test first holds, or after nt steps --
//     its lane writes one cbet_ray_exit record.  GAIN: the CBET hook of k_trace_window<16, ., 1> -- that kernel's own code,
//     cbet_trace_common.h -- before the absorption, so that a ray's exit energy is what the CBET deposition pass leaves it.
//     The step is one function, ray_step of cbet_trace_common.h, which the path recorder (cbet_trace_path.hip) calls too;
//     what is here is the kernel's own: the bundle prologue, the exit record, the counters.
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

template <bool GAIN, bool IDX64>
__global__ void __launch_bounds__(kWave) k_trace_exit(const TraceArgs a)
{
    const int lane = threadIdx.x;
    int beam, patch;
    if (!work_item(a, blockIdx.x, beam, patch)) return;   // wave-uniform

    Ray s = {};
    int li;
    const bool launched = launch_lane(a, beam, patch, lane, s, li);
    const bool has_slot = li < a.nlive;                   // (a record for every slot of the list, idle lanes' too)
    const double uray0 = s.uray;                          // :113

    // (a beam's bundle: one gain grid for the wave)
    const StepFrame f = step_frame(a, lane, GAIN ? a.gain + (long)(beam - a.grid_beam0) * a.hsize : nullptr);
    StepRecord rec = {0.0, 0.0, 0.0, 0.0};
    unsigned cell = 0;
    if (launched) rec = load_record<IDX64>(a, node_of(f, s));   // :254-270 at the launch node
    double absorbed = 0.0, gained = 0.0;                  // (absorbed: not taken, the records give it as a difference)

    bool alive = launched;
    int steps = 0, status = 0;
    for (int tt = 0; tt < a.nt; ++tt) {                   // :207
        if (__builtin_amdgcn_ballot_w64(alive) == 0ull) break;
        // the six planes through a.bounds: nothing is stored in this loop, so the loads are scalar ones
        const int end = ray_step<GAIN, IDX64, false>(a, f, a.bounds, alive, s, rec, cell, absorbed, gained);
        if (__builtin_expect(end != 0, 0)) {              // (once per ray: kept a branch, not selects in every step)
            alive = false;
            steps = tt + 1;
            status = CBET_RAY_LAUNCHED | end;
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

    count_steps_and_rays(a, lane, steps, launched);
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
    return launch_gain_by_index(a, force_idx64, [&](auto gain, auto wide) {
        hipLaunchKernelGGL((k_trace_exit<gain, wide>), grid, block, 0, stream, a);
    });
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
