// cbet_trace_path.hip -- the ray path recorder for gfx950 (CDNA4): sampled trajectories and one closest-approach record
// per ray, for an explicit list of rays (include/cbet_mi355x.h cbet_trace_paths).
//
//   * k_trace_path<GAIN, IDX64> : a sibling of k_trace_exit (cbet_trace_exit.hip).  One wavefront = 64 consecutive items of
//     the caller's list, lane l of workgroup w takes item 64 w + l.  Kick, drift, nearest-node update, step-record gather,
//     the CBET hook, absorption and the stop test are one function, ray_step of cbet_trace_common.h, which that kernel
//     calls too, so a ray's position, node, energy, step count and status are the exit pass's by construction.  What is
//     here is the recorder's own: the item decoding; per step the squared distance to the centre, one compare and the
//     selects that remember the closest approach; every `stride` steps, and in the step a ray ends, a 64-byte sample with
//     its step-order sums; the turn record.  Samples are sample-major (samples[m][item]): the 64 lanes of a wave write
//     4 KB of consecutive whole lines per sampled step.
//
// Nothing here is hand-scheduled, and the context's counters are not touched.
#include <hip/hip_runtime.h>

#include "cbet_trace_common.h"

namespace cbet {

static_assert(sizeof(cbet_path_sample) == 64 && sizeof(cbet_ray_turn) == 64, "path records are 64 bytes (include/cbet_mi355x.h)");

namespace {

// Sample m of `item`, if the caller's array holds it: the guard is per store and unconditional.
__device__ __forceinline__ void store_sample(const TraceArgs &a, const PathArgs &q, long item, int m, const Ray &s, double absorbed,
                                             double gained, int step)
{
    if (!(m >= 0 && m < q.capacity)) return;
    cbet_path_sample *const dst = q.samples + ((long)m * q.nitems + item);
#ifdef CBET_DEBUG_BOUNDS
    if (!(dst >= q.audit_samples_lo && dst + 1 <= q.audit_samples_hi)) { audit_fail(a); return; }
#else
    (void)a;
#endif
    cbet_path_sample r;
    r.x = s.px; r.y = s.py; r.z = s.pz;
    r.uray = s.uray; r.absorbed = absorbed; r.gained = gained;
    r.ci = s.ci; r.cj = s.cj; r.ck = s.ck; r.step = step;
    *dst = r;
}

// include/cbet_mi355x.h cbet_ray_turn: that parenthesisation, one IEEE operation per statement (-ffp-contract=off)
__device__ __forceinline__ double distance2(const PathArgs &q, const Ray &s)
{
    const double ex = s.px - q.cx, ey = s.py - q.cy, ez = s.pz - q.cz;
    return (ex * ex + ey * ey) + ez * ez;
}

template <bool GAIN, bool IDX64>
__global__ void __launch_bounds__(kWave) k_trace_path(const TraceArgs a, const PathArgs q)
{
    const int lane = threadIdx.x;
    const long item = (long)blockIdx.x * kWave + lane;
    const bool has_item = item < q.nitems;

    // the item's ray, decoded only when both ids are in range: every raynum in [0, nrays) indexes the launch axes in
    // range (the header's derivation), nothing else may reach launch_ray
    int beam = 0, raynum = -1;
    if (has_item) { beam = q.beams[item]; raynum = q.raynums[item]; }
    const bool valid = has_item && beam >= 0 && beam < q.nbeams && raynum >= 0 && raynum < q.nrays;
    Ray s = {};
    const bool launched = valid && launch_ray(a, beam, raynum, s);

    // a wave may hold several beams: the gain base is per lane
    const StepFrame f = step_frame(a, lane, (GAIN && launched) ? a.gain + (long)beam * a.hsize : a.gain);
    StepRecord rec = {0.0, 0.0, 0.0, 0.0};
    unsigned cell = 0;
    if (launched) {
        cell = node_of(f, s);
        rec = load_record<IDX64>(a, cell);                   // :254-270 at the launch node
    }

    // sample 0 and the closest approach so far: the launch state
    if (launched) store_sample(a, q, item, 0, s, 0.0, 0.0, 0);
    double best_r2 = 0.0, best_x = 0.0, best_y = 0.0, best_z = 0.0, best_u = 0.0;
    unsigned best_cell = 0;
    int best_step = 0;
    if (launched) {
        best_r2 = distance2(q, s);
        best_x = s.px; best_y = s.py; best_z = s.pz; best_u = s.uray;
        best_cell = cell;
    }

    double absorbed = 0.0, gained = 0.0;                     // since the previous sample, in step order
    int whole = 0, phase = 0;                                // wave-uniform: (tt + 1) / stride and (tt + 1) % stride

    bool alive = launched;
    int steps = 0, status = 0;
    for (int tt = 0; tt < a.nt; ++tt) {                      // :207
        if (__builtin_amdgcn_ballot_w64(alive) == 0ull) break;
        if (++phase == q.stride) { phase = 0; ++whole; }
        const bool stepping = alive;
        // The six planes come from the argument segment (TraceArgs::exit_planes, the values of a.bounds by
        // host_exit_planes): this loop stores to memory, so the compiler could keep loads through a.bounds neither scalar
        // nor out of the loop -- six vector loads and their wait in every step (measured at 256^3: 1.68 x the exit pass
        // that way, 1.03 x this way).  absorbed, gained: the sums since the previous sample, taken by lanes that step.
        const int end = ray_step<GAIN, IDX64, true>(a, f, a.exit_planes, alive, s, rec, cell, absorbed, gained);
        if (__builtin_expect(end != 0, 0)) {                 // (once per ray, as in k_trace_exit)
            alive = false;
            steps = tt + 1;
            status = CBET_RAY_LAUNCHED | end;
        }
        if (stepping) {
            // the closest approach: the first minimum wins
            const double r2 = distance2(q, s);
            if (r2 < best_r2) {
                best_r2 = r2;
                best_x = s.px; best_y = s.py; best_z = s.pz; best_u = s.uray;
                best_cell = cell;
                best_step = tt + 1;
            }
            // a sample after every stride-th step, and of the end state
            if (phase == 0 || !alive) {
                store_sample(a, q, item, phase == 0 ? whole : whole + 1, s, absorbed, gained, tt + 1);
                absorbed = 0.0;
                gained = 0.0;
            }
        }
    }
    if (alive) {                                             // ran out of steps (:207)
        steps = a.nt;
        status = CBET_RAY_LAUNCHED | CBET_RAY_TIMEOUT;
        if (phase != 0) store_sample(a, q, item, whole + 1, s, absorbed, gained, steps);   // the end state, once
    }

    if (has_item) {
        cbet_ray_turn t = {};
        if (launched) {
            t.r2 = best_r2;
            t.x = best_x; t.y = best_y; t.z = best_z; t.uray = best_u;
            t.ne = node_load<IDX64>(a, a.ne3d, best_cell, a.audit_nodes);
            t.step = best_step; t.steps = steps; t.status = status;
            t.nsamples = 1 + (steps + q.stride - 1) / q.stride;
        }
        cbet_ray_turn *const dst = q.turns + item;
#ifdef CBET_DEBUG_BOUNDS
        if (!(dst >= q.audit_turns_lo && dst + 1 <= q.audit_turns_hi)) audit_fail(a);
        else
#endif
        *dst = t;
    }
}

}  // namespace

hipError_t launch_trace_path(const TraceArgs &a, const PathArgs &q0, bool force_idx64, hipStream_t stream)
{
    if (q0.nitems <= 0) return hipSuccess;
    PathArgs q = q0;
#ifdef CBET_DEBUG_BOUNDS
    q.audit_samples_lo = q.samples; q.audit_samples_hi = q.samples + (long)q.capacity * q.nitems;
    q.audit_turns_lo = q.turns; q.audit_turns_hi = q.turns + q.nitems;
#endif
    const dim3 grid((unsigned)((q.nitems + kWave - 1) / kWave)), block(kWave);
    return launch_gain_by_index(a, force_idx64, [&](auto gain, auto wide) {
        hipLaunchKernelGGL((k_trace_path<gain, wide>), grid, block, 0, stream, a, q);
    });
}

}  // namespace cbet
