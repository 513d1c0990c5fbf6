// cbet_backscatter.hip -- backscatter SBS gain spectra along rays for gfx950 (CDNA4): include/cbet_mi355x.h
// cbet_trace_backscatter and cbet_backscatter_tally, DESIGN.md section 24.  No reference counterpart: parity unpinned.
//
//   * k_trace_backscatter<GAIN, IDX64, NS> : a sibling of k_trace_path (cbet_trace_path.hip).  One wavefront = 64 consecutive
//     items of the caller's list, decoded as there; the step is ray_step of cbet_trace_common.h, which the exit pass and the
//     path recorder call too, so a ray's positions, nodes, energy, step count and status are theirs by construction.  What is
//     here is the spectrum's own: per stepping lane three subtractions against the kept previous position, then the model of
//     cbet_sbs_model.h -- path length, ion-acoustic wave, the cell's state and prefactor (cell_state's run-time-selecting
//     overload: the flow and state tables are chosen by the block), and per shift the gain stage's detuned pair gain into one
//     of NS register accumulators.  Slots >= nshift are skipped by a wave-uniform test; the shifts are read by scalar loads from
//     the argument segment, once, and kept in the lanes of one register pair.  The loop stores nothing: gamma (shift-major, a wave writes whole lines) and the 32-byte records are
//     written once, behind it.
//   * k_backscatter_tally + k_backscatter_reduce : per beam and shift {sum uray0, sum uray0 Gamma, max Gamma, rays} over the
//     launched items, without atomics -- fixed-order partial entries per chunk of the list in a work buffer, then a
//     fixed-order second stage that merges them into the caller's table, as k_lpi_reduce does.
//
// Nothing here is hand-scheduled, no LDS is used, and the context's counters are not touched.
#include <hip/hip_runtime.h>

#include "cbet_sbs_model.h"
#include "cbet_trace_common.h"

namespace cbet {

static_assert(sizeof(cbet_ray_sbs) == 32, "cbet_ray_sbs is 32 bytes (include/cbet_mi355x.h)");

namespace {

// Gamma_m of `item`, if the caller's array holds it: the guard is per store and unconditional.
__device__ __forceinline__ void store_gamma(const TraceArgs &a, const SbsArgs &q, long item, int m, double v)
{
    if (!(m >= 0 && m < q.nshift && item >= 0 && item < q.nitems)) return;
    double *const dst = q.gamma + ((long)m * q.nitems + item);
#ifdef CBET_DEBUG_BOUNDS
    if (!(dst >= q.audit_gamma_lo && dst + 1 <= q.audit_gamma_hi)) { audit_fail(a); return; }
#else
    (void)a;
#endif
    *dst = v;
}

__device__ __forceinline__ void store_ray(const TraceArgs &a, const SbsArgs &q, long item, const cbet_ray_sbs &r)
{
    if (!(item >= 0 && item < q.nitems)) return;
    cbet_ray_sbs *const dst = q.rays + item;
#ifdef CBET_DEBUG_BOUNDS
    if (!(dst >= q.audit_rays_lo && dst + 1 <= q.audit_rays_hi)) { audit_fail(a); return; }
#else
    (void)a;
#endif
    *dst = r;
}

// Lane m's double, as a wave-uniform value (two v_readlane_b32, m a constant).
__device__ __forceinline__ double lane_value(double v, int m)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), m), __builtin_amdgcn_readlane(__double2loint(v), m));
}

// A loop-invariant uniform double kept in a vector register pair from here on (an empty statement the compiler cannot see through).
__device__ __forceinline__ double in_vgpr(double x)
{
    asm volatile("" : "+v"(x));
    return x;
}

// Scalar registers.  The three blocks are 100+ loop-invariant scalars and every unrolled quotient wants a
// condition-register pair in flight; what does not fit the 102 registers is spilled to lanes of a vector register -- and the
// first build's listing then reported a 36-byte private segment that no instruction touched.  Three things in the kernel's
// first lines keep every instantiation without one (some lane spills remain):
//   * the grid's sides and origin, the density table and ncrit are the trace's own (gain_args and trace_impl fill both blocks
//     from the same cbet_params / cbet_derived and the same table): the model's block is a copy of `g0` with those members
//     taken from `a`, so they are held once;
//   * the shifts are read once, by scalar loads, into lane m of ONE vector register pair, and a step reads shift m back as a
//     uniform value (lane_value): 2 NS scalar registers less;
//   * thirteen loop-invariant doubles of the model live in vector registers (in_vgpr).
template <bool GAIN, bool IDX64, int NS>
__global__ void __launch_bounds__(kWave) k_trace_backscatter(const TraceArgs a, const GainArgs g0, const SbsArgs q)
{
    GainArgs g = g0;
    g.nx = a.nx; g.ny = a.ny; g.nz = a.nz;
    g.xmin = a.xmin; g.ymin = a.ymin; g.zmin = a.zmin;
    g.ne3d = a.ne3d;
    g.dx = in_vgpr(a.dx); g.dy = in_vgpr(a.dy); g.dz = in_vgpr(a.dz);
    g.ncrit = in_vgpr(a.ncrit);
    g.cs = in_vgpr(g0.cs); g.gain_const = in_vgpr(g0.gain_const); g.iaw = in_vgpr(g0.iaw);
    g.mach_r0 = in_vgpr(g0.mach_r0); g.mach_0 = in_vgpr(g0.mach_0); g.mach_r1 = in_vgpr(g0.mach_r1); g.mach_1 = in_vgpr(g0.mach_1);
    const double qs = in_vgpr(q.qs), iaw2 = in_vgpr(q.iaw2);
    const int lane = threadIdx.x;
    double shift_of_lane = 0.0;
#pragma unroll
    for (int m = 0; m < NS; ++m)
        if (lane == m) shift_of_lane = q.shifts[m];
    const long item = (long)blockIdx.x * kWave + lane;
    const bool has_item = item < q.nitems;

    // the item's ray, decoded only when both ids are in range (k_trace_path's rule)
    int beam = 0, raynum = -1;
    if (has_item) { beam = q.beams[item]; raynum = q.raynums[item]; }
    const bool valid = has_item && beam >= 0 && beam < q.nbeams && raynum >= 0 && raynum < q.nrays;
    Ray s = {};
    const bool launched = valid && launch_ray(a, beam, raynum, s);

    // a wave may hold several beams: the gain base and the intensity base are per lane
    const StepFrame f = step_frame(a, lane, (GAIN && launched) ? a.gain + (long)beam * a.hsize : a.gain);
    const double *const fI = g.fields + (launched ? (long)beam * g.bstride : 0L);
    StepRecord rec = {0.0, 0.0, 0.0, 0.0};
    unsigned cell = 0;
    if (launched) {
        cell = node_of(f, s);
        rec = load_record<IDX64>(a, cell);
    }
    const double uray0 = launched ? s.uray : 0.0;
    double px = s.px, py = s.py, pz = s.pz;                  // p_(t-1)
    const bool smoothed = g.pol != 0;

    double gam[NS];
#pragma unroll
    for (int m = 0; m < NS; ++m) gam[m] = 0.0;

    double absorbed = 0.0, gained = 0.0;                     // (ray_step's sums; not reported here)
    bool alive = launched;
    int steps = 0, status = 0;
    for (int tt = 0; tt < a.nt; ++tt) {
        if (__builtin_amdgcn_ballot_w64(alive) == 0ull) break;
        const bool stepping = alive;
        const int end = ray_step<GAIN, IDX64, false>(a, f, a.exit_planes, alive, s, rec, cell, absorbed, gained);
        if (__builtin_expect(end != 0, 0)) {
            alive = false;
            steps = tt + 1;
            status = CBET_RAY_LAUNCHED | end;
        }
        if (stepping) {
            const double dx = s.px - px, dy = s.py - py, dz = s.pz - pz;
            px = s.px; py = s.py; pz = s.pz;
            const SbsStep t = sbs_step(qs, dx, dy, dz);
            if (t.ds != 0.0) {
                const long h = sbs_cell(g, s.ci, s.cj, s.ck);
                const CellState c = cell_state(g, h);
                const double pref = cell_pref(g, c);
                const double I = fI[h];
#pragma unroll
                for (int m = 0; m < NS; ++m)
                    if (m < q.nshift) gam[m] = sbs_add(gam[m], sbs_gain(c, pref, iaw2, t.w, lane_value(shift_of_lane, m), smoothed), I, t.ds);
            }
        }
    }
    if (alive) {                                             // ran out of steps
        steps = a.nt;
        status = CBET_RAY_LAUNCHED | CBET_RAY_TIMEOUT;
    }

    if (has_item) {
        cbet_ray_sbs r = {};
        if (launched) {
            double gmax = 0.0;
            int imax = 0;
#pragma unroll
            for (int m = 0; m < NS; ++m)
                if (m < q.nshift) sbs_max(gam[m], m, gmax, imax);
            r.gmax = gmax; r.uray0 = uray0; r.uray_end = s.uray;
            r.steps = steps; r.imax = (short)imax; r.status = (short)status;
        }
        store_ray(a, q, item, r);
#pragma unroll
        for (int m = 0; m < NS; ++m)
            if (m < q.nshift) store_gamma(a, q, item, m, launched ? gam[m] : 0.0);
    }
}

// ---- the per-beam tally -------------------------------------------------------------------------------------------------
struct SbsTally { double u, ug, mx, n; };                   // sum uray0, sum uray0 Gamma, max Gamma (0 while n == 0), rays
// Sums and counts add, the maximum is taken over sides that count a ray.  Every operation commutes, so the two lanes of a
// butterfly pair end with the same bits.
__device__ __forceinline__ void tally_merge(SbsTally &s, const SbsTally &t)
{
    s.mx = s.n == 0.0 ? t.mx : (t.n == 0.0 ? s.mx : (t.mx > s.mx ? t.mx : s.mx));
    s.u = s.u + t.u;
    s.ug = s.ug + t.ug;
    s.n = s.n + t.n;
}
__device__ __forceinline__ void tally_wave_merge(SbsTally &s)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        SbsTally t;
        t.u = __shfl_xor(s.u, off, kWave); t.ug = __shfl_xor(s.ug, off, kWave);
        t.mx = __shfl_xor(s.mx, off, kWave); t.n = __shfl_xor(s.n, off, kWave);
        tally_merge(s, t);
    }
}
// The item's beam if the item counts: a launched record of a beam in range; -1 otherwise.
__device__ __forceinline__ int tally_beam(const cbet_ray_sbs *rays, const int *beams, long k, int nbeams)
{
    const int b = beams[k];
    return (b >= 0 && b < nbeams && (rays[k].status & CBET_RAY_LAUNCHED) != 0) ? b : -1;
}

// One wavefront per (chunk, shift): lane l takes the chunk's items l, l + 64, ... in that order, beam by beam over the beams
// the chunk holds (a bit mask, OR-ed across the lanes: nbeams <= CBET_MAX_CBET_BEAMS = 64), six butterfly steps merge the lanes, lane 0
// stores the entry work[chunk][shift][beam] -- zeros for a beam the chunk does not hold.  Every entry of `work` is written.
__global__ void __launch_bounds__(kWave) k_backscatter_tally(const double *__restrict__ gamma, const cbet_ray_sbs *__restrict__ rays,
                                                             const int *__restrict__ beams, long nitems, int nshift, int nbeams,
                                                             long chunk_items, double *__restrict__ work)
{
    const int lane = threadIdx.x;
    const long chunk = blockIdx.x;
    const int m = blockIdx.y;
    const long lo = chunk * chunk_items, hi = lo + chunk_items < nitems ? lo + chunk_items : nitems;
    unsigned long long mask = 0ull;
    for (long k = lo + lane; k < hi; k += kWave) {
        const int b = tally_beam(rays, beams, k, nbeams);
        if (b >= 0) mask |= 1ull << b;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mask |= (unsigned long long)__shfl_xor((long long)mask, off, kWave);
    const double *const gm = gamma + (long)m * nitems;
    for (int b = 0; b < nbeams; ++b) {
        SbsTally s = {0.0, 0.0, 0.0, 0.0};
        if ((mask >> b) & 1ull) {                            // wave-uniform
            for (long k = lo + lane; k < hi; k += kWave) {
                if (tally_beam(rays, beams, k, nbeams) != b) continue;
                const double u = rays[k].uray0, G = gm[k];
                const SbsTally t = {u, u * G, G, 1.0};
                tally_merge(s, t);
            }
            tally_wave_merge(s);
        }
        if (lane == 0) {
            double *const dst = work + (((long)chunk * nshift + m) * nbeams + b) * CBET_SBS_TALLY_COLUMNS;
            dst[CBET_SBS_TALLY_URAY0] = s.u; dst[CBET_SBS_TALLY_WEIGHTED] = s.ug;
            dst[CBET_SBS_TALLY_MAX] = s.mx; dst[CBET_SBS_TALLY_N_RAYS] = s.n;
        }
    }
}

// One wavefront per (beam, shift): lane l merges the chunks l, l + 64, ... in that order, six butterfly steps merge the
// lanes, lane 0 merges the result into the caller's entry.  A fixed order for a given nitems: two calls give the same bits.
__global__ void __launch_bounds__(kWave) k_backscatter_reduce(const double *__restrict__ work, long chunks, int nshift, int nbeams,
                                                              double *__restrict__ tally)
{
    const int b = blockIdx.x, m = blockIdx.y;
    SbsTally s = {0.0, 0.0, 0.0, 0.0};
    for (long c = threadIdx.x; c < chunks; c += kWave) {
        const double *const src = work + ((c * nshift + m) * nbeams + b) * CBET_SBS_TALLY_COLUMNS;
        const SbsTally t = {src[CBET_SBS_TALLY_URAY0], src[CBET_SBS_TALLY_WEIGHTED], src[CBET_SBS_TALLY_MAX], src[CBET_SBS_TALLY_N_RAYS]};
        tally_merge(s, t);
    }
    tally_wave_merge(s);
    if (threadIdx.x == 0) {
        double *const dst = tally + ((long)b * nshift + m) * CBET_SBS_TALLY_COLUMNS;
        SbsTally t = {dst[CBET_SBS_TALLY_URAY0], dst[CBET_SBS_TALLY_WEIGHTED], dst[CBET_SBS_TALLY_MAX], dst[CBET_SBS_TALLY_N_RAYS]};
        tally_merge(t, s);
        dst[CBET_SBS_TALLY_URAY0] = t.u; dst[CBET_SBS_TALLY_WEIGHTED] = t.ug;
        dst[CBET_SBS_TALLY_MAX] = t.mx; dst[CBET_SBS_TALLY_N_RAYS] = t.n;
    }
}

template <int NS>
hipError_t launch_ns(const TraceArgs &a, const GainArgs &g, const SbsArgs &q, bool force_idx64, hipStream_t stream)
{
    const dim3 grid((unsigned)((q.nitems + kWave - 1) / kWave)), block(kWave);
    return launch_gain_by_index(a, force_idx64, [&](auto gain, auto wide) {
        hipLaunchKernelGGL((k_trace_backscatter<gain, wide, NS>), grid, block, 0, stream, a, g, q);
    });
}

}  // namespace

hipError_t launch_trace_backscatter(const TraceArgs &a, const GainArgs &g, const SbsArgs &q0, bool force_idx64, hipStream_t stream)
{
    if (q0.nitems <= 0) return hipSuccess;
    if (q0.nshift < 1 || q0.nshift > CBET_SBS_MAX_SHIFTS) return hipErrorInvalidValue;
    SbsArgs q = q0;
#ifdef CBET_DEBUG_BOUNDS
    q.audit_gamma_lo = q.gamma; q.audit_gamma_hi = q.gamma + (long)q.nshift * q.nitems;
    q.audit_rays_lo = q.rays; q.audit_rays_hi = q.rays + q.nitems;
#endif
    if (q.nshift <= 4) return launch_ns<4>(a, g, q, force_idx64, stream);
    if (q.nshift <= 8) return launch_ns<8>(a, g, q, force_idx64, stream);
    return launch_ns<CBET_SBS_MAX_SHIFTS>(a, g, q, force_idx64, stream);
}

hipError_t launch_backscatter_tally(const double *gamma, const cbet_ray_sbs *rays, const int *beams, long nitems, int nshift,
                                    int nbeams, double *tally, double *work, hipStream_t stream)
{
    if (nitems <= 0 || nshift <= 0 || nbeams <= 0) return hipSuccess;
    const long chunks = sbs_chunks(nitems);
    hipLaunchKernelGGL(k_backscatter_tally, dim3((unsigned)chunks, (unsigned)nshift), dim3(kWave), 0, stream, gamma, rays, beams,
                       nitems, nshift, nbeams, sbs_chunk_items(nitems), work);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_backscatter_reduce, dim3((unsigned)nbeams, (unsigned)nshift), dim3(kWave), 0, stream, work, chunks, nshift,
                       nbeams, tally);
    return hipGetLastError();
}

}  // namespace cbet
