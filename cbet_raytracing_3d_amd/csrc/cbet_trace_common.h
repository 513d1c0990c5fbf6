// cbet_trace_common.h -- what the ray-integrator kernels share, each piece of a ray step stated once (cbet_kernels.hip: the two
// cross-check formulations; cbet_trace_window.hip: the shipped one; cbet_trace_exit.hip: the exit pass; cbet_trace_path.hip: the path recorder).  Citations are into /root/reference/.
// Everything here is compiled with -ffp-contract=off: one IEEE operation per reference statement.
#ifndef CBET_TRACE_COMMON_H_
#define CBET_TRACE_COMMON_H_

#include <hip/hip_runtime.h>

#include <type_traits>

#include "cbet_device.h"
#include "cbet_relocate.h"

namespace cbet {

// ---------------------------------------------------------------------------------------------
// launch_ray_XZ.cu:16-63 -- clamped piecewise-linear lookup, bisection; both abscissa orders.
// (The node tables' lookups share one bracket, cbet_node_model.h; written over it the trace kernels compile differently.)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double interp_table(const double *y, const double *x, const double xp, int n)
{
    unsigned lo, hi, mid;
    if (x[0] <= x[n - 1]) {
        if (xp <= x[0]) return y[0];
        if (xp >= x[n - 1]) return y[n - 1];
        lo = 0;
        hi = n - 1;
        mid = (lo + hi) >> 1;
        while (lo < hi - 1) {
            if (x[mid] >= xp) hi = mid; else lo = mid;
            mid = (lo + hi) >> 1;
        }
    } else {
        if (xp >= x[0]) return y[0];
        if (xp <= x[n - 1]) return y[n - 1];
        lo = 0;
        hi = n - 1;
        mid = (lo + hi) >> 1;
        while (lo < hi - 1) {
            if (x[mid] <= xp) lo = mid; else hi = mid;
            mid = (lo + hi) >> 1;
        }
    }
    return y[mid] + (y[mid + 1] - y[mid]) / (x[mid + 1] - x[mid]) * (xp - x[mid]);
}

struct Ray {
    double px, py, pz, vx, vy, vz, uray, ustop;
    int ci, cj, ck;
};

// First node q in [0,n) with |q*d+lo - p| <= tol, else 0 (launch_ray_XZ.cu:162-180).  Only nodes
// next to p can satisfy the predicate, so the upward scan is restricted to a 5-node window; the
// predicate itself is the reference's.
__device__ __forceinline__ int first_node_within(double p, double lo, double d, double tol, int n)
{
    double f = (p - lo) / d;
    int g = (f > -4.0 && f < (double)n + 4.0) ? (int)floor(f) : -8;
    int found = 0;
    bool have = false;
    for (int q = g - 2; q <= g + 2; ++q) {
        if (q < 0 || q >= n || have) continue;
        if (fabs(q * d + lo - p) <= tol) {
            found = q;
            have = true;
        }
    }
    return found;
}

// launch_ray_XZ.cu:65-115 + :162-204 : launch point, power, first cell, launch wave-vector.
__device__ __forceinline__ bool launch_ray(const TraceArgs &a, int beam, int pre_raynum, Ray &s)
{
    const int rpz = a.rpz, rpz2 = rpz * rpz;
    const int tile = pre_raynum / rpz2, within = pre_raynum % rpz2;   // :70-71
    const int ry = tile / a.zones * rpz + within / rpz;               // :72
    const int rx = tile % a.zones * rpz + within % rpz;               // :73
    // :76-92 the repeated-addition loops are tabulated on the host (same additions, same order)
    double x0 = a.xlaunch[rx];
    double y0 = a.ylaunch[ry];
    const double ref = sqrt(x0 * x0 + y0 * y0);                       // :94
    double z0 = a.z_launch;                                           // :97

    const double bnx = a.beam_norm[beam * 3 + 0], bny = a.beam_norm[beam * 3 + 1],
                 bnz = a.beam_norm[beam * 3 + 2];
    double c1, s1, c2, s2;
    if (a.bbeam_norm) {  // main.cu:121-129 host trig, 4 per beam
        c1 = a.bbeam_norm[4 * beam + 0];
        s1 = a.bbeam_norm[4 * beam + 1];
        c2 = a.bbeam_norm[4 * beam + 2];
        s2 = a.bbeam_norm[4 * beam + 3];
    } else {             // :99-100 on the device
        const double theta1 = acos(bnz);
        const double theta2 = atan2(bny * kFocal, kFocal * bnx);
        c1 = cos(theta1);
        s1 = sin(theta1);
        c2 = cos(theta2);
        s2 = sin(theta2);
    }
    const double keep = x0;                                           // :102-111
    x0 = x0 * c1 + z0 * s1;
    z0 = z0 * c1 - keep * s1;
    const double keep2 = x0;
    x0 = x0 * c2 - y0 * s2;
    y0 = y0 * c2 + keep2 * s2;

    s.px = x0;
    s.py = y0;
    s.pz = z0;
    s.uray = a.uray_mult * interp_table(a.pow_r, a.phase_r, ref, CBET_NPHASE);  // :113
    s.ustop = 0.05 * s.uray;                                                    // :351
    if (!(ref <= kBeamMax)) return false;                                       // :114

    s.ci = first_node_within(s.px, a.xmin, a.dx, a.tol_x, a.nx);      // :162-180
    s.cj = first_node_within(s.py, a.ymin, a.dy, a.tol_y, a.ny);
    s.ck = first_node_within(s.pz, a.zmin, a.dz, a.tol_z, a.nz);

    // :186-204 ne at the launch node == the tabulated node value
    const double ne0 = a.ne3d[((long)s.ci * a.ny + s.cj) * a.nz + s.ck];
    const double w = sqrt((a.omega * a.omega - ne0 * 1e6 * (kEc * kEc) / ((double)kMe * kE0)) / (kC * kC));
    double vx = -1 * bnx, vy = -1 * bny, vz = -1 * bnz;
    const double knorm = sqrt(vx * vx + vy * vy + vz * vz);
    s.vx = (kC * kC) * ((vx / knorm) * w) / a.omega;
    s.vy = (kC * kC) * ((vy / knorm) * w) / a.omega;
    s.vz = (kC * kC) * ((vz / knorm) * w) / a.omega;
    return true;
}

// The bundle prologue of every integrator: the lane takes slot li of the launch list (whole bundles: the test against its
// end is a guard only); -1 there is a hole in the 8x8 patch.  False for a hole and for a ray culled at :114.
__device__ __forceinline__ bool launch_lane(const TraceArgs &a, int beam, int patch, int lane, Ray &s, int &li)
{
    li = patch * kWave + lane;
    const int pre_raynum = li < a.nlive ? a.live[li] : -1;
    return pre_raynum >= 0 && launch_ray(a, beam, pre_raynum, s);
}

// launch_ray_XZ.cu:212-238 -- the two nodes whose ne difference kicks a ray at node c of an axis of n nodes, as offsets from
// c in units of `stride`: this -+ 1, one-sided on the faces (0 -> (0, 2), n-1 -> (n-3, n-1)).  Table kernels and k_trace_simple.
template <class T = int> __device__ __forceinline__ void face_pair(int c, int n, T &m, T &p, T stride = 1)
{
    m = (c == 0) ? 0 : ((c == n - 1) ? -2 * stride : -stride);
    p = (c == 0) ? 2 * stride : ((c == n - 1) ? 0 : stride);
}

// launch_ray_XZ.cu:271-278 -- drift with the kicked velocity, then the position in cell units.
__device__ __forceinline__ void drift(const TraceArgs &a, Ray &s, double &fx, double &fy, double &fz)
{
    s.px += s.vx * a.dt; s.py += s.vy * a.dt; s.pz += s.vz * a.dt;
    fx = (s.px - a.xmin) * a.inv_dx; fy = (s.py - a.ymin) * a.inv_dy; fz = (s.pz - a.zmin) * a.inv_dz;
}

// launch_ray_XZ.cu:351-356 -- the stop test's two conditions as status bits: the energy cut-off (CBET_RAY_CUTOFF), a position
// outside the six exit planes b = {xlo, xhi, ylo, yhi, zlo, zhi} of TraceArgs::bounds (CBET_RAY_ESCAPED).  0: the ray goes on.
__device__ __forceinline__ int stop_test(const Ray &s, const double *b)
{
    const bool out = s.px < b[0] || s.px > b[1] || s.py < b[2] || s.py > b[3] || s.pz < b[4] || s.pz > b[5];
    return (s.uray <= s.ustop ? CBET_RAY_CUTOFF : 0) | (out ? CBET_RAY_ESCAPED : 0);
}

// Bounds-audited build (tests/test_gpu_bounds_audit.py, -DCBET_DEBUG_BOUNDS): every grid atomic, node-table
// gather and LDS accumulate is range-checked against the limits the launch put into TraceArgs; a violation
// is counted and the access skipped.  Never shipped.
#ifdef CBET_DEBUG_BOUNDS
__device__ __forceinline__ bool audit_fail(const TraceArgs &a)
{
    atomicAdd(a.audit_count, 1ull);
    return true;
}
#define CBET_AUDIT(a, cond) ((cond) || !audit_fail(a))
#else
#define CBET_AUDIT(a, cond) true
#endif

__device__ __forceinline__ void global_add(const TraceArgs &a, double *p, double v)
{
#ifdef CBET_DEBUG_BOUNDS
    if (!(p >= a.audit_lo && p < a.audit_hi)) { audit_fail(a); return; }
#else
    (void)a;
#endif
    // native global_atomic_add_f64, no CAS loop (checked in the ISA)
    unsafeAtomicAdd(p, v);
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// Ray-steps and rays of a bundle into the device counters: one atomic per wave and counter.
__device__ __forceinline__ void count_steps_and_rays(const TraceArgs &a, int lane, int steps, bool launched)
{
    const int tot_steps = wave_sum(launched ? steps : 0), tot_rays = wave_sum(launched ? 1 : 0);
    if (lane == 0) {
        atomicAdd(&a.counters[kCntSteps], (unsigned long long)tot_steps);
        atomicAdd(&a.counters[kCntRays], (unsigned long long)tot_rays);
    }
}

// 8-byte gather from a node table, or from a beam's haloed gain grid (CBET hooks), by 32-bit element index: uniform base +
// zero-extended 32-bit byte offset, which the backend turns into the saddr+voffset form of global_load_dwordx2 (no 64-bit
// address arithmetic per lane).  Valid while 8*nodes < 2^32 (checked on the host).  bound: the table's entries, which the
// bounds-audited build checks the index against (TraceArgs.audit_nodes, audit_hsize).
template <bool IDX64>
__device__ __forceinline__ double node_load(const TraceArgs &a, const double *base, unsigned idx, unsigned long long bound)
{
#ifdef CBET_DEBUG_BOUNDS
    if (!(idx < bound)) { audit_fail(a); return 0.0; }
#else
    (void)a; (void)bound;
#endif
    if (IDX64) return base[idx];
    return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(base) + (idx * 8u));
}

// Two z-adjacent entries (idx, idx + 1) of the gain grid in ONE 16-byte gather (8-byte aligned: the hardware takes it).
typedef double gain_pair_t __attribute__((ext_vector_type(2), aligned(8)));
template <bool IDX64>
__device__ __forceinline__ gain_pair_t gain_load2(const TraceArgs &a, const double *base, unsigned idx)
{
#ifdef CBET_DEBUG_BOUNDS
    if (!(idx + 1u < a.audit_hsize)) { audit_fail(a); return gain_pair_t{0.0, 0.0}; }
#else
    (void)a;
#endif
    if (IDX64) return *reinterpret_cast<const gain_pair_t *>(base + idx);
    return *reinterpret_cast<const gain_pair_t *>(reinterpret_cast<const char *>(base) + (idx * 8u));
}

// phi(x) = (exp(x) - 1) / x, |x| <= 1: degree-17 Horner polynomial of plain multiplies and adds, the
// operation sequence the CPU checker of the CBET stage evaluates.  CBET extension only.
__device__ __forceinline__ double phi_det(double x)
{
    double p = 1.0 / 6402373705728000.0;
    p = p * x + 1.0 / 355687428096000.0;
    p = p * x + 1.0 / 20922789888000.0;
    p = p * x + 1.0 / 1307674368000.0;
    p = p * x + 1.0 / 87178291200.0;
    p = p * x + 1.0 / 6227020800.0;
    p = p * x + 1.0 / 479001600.0;
    p = p * x + 1.0 / 39916800.0;
    p = p * x + 1.0 / 3628800.0;
    p = p * x + 1.0 / 362880.0;
    p = p * x + 1.0 / 40320.0;
    p = p * x + 1.0 / 5040.0;
    p = p * x + 1.0 / 720.0;
    p = p * x + 1.0 / 120.0;
    p = p * x + 1.0 / 24.0;
    p = p * x + 1.0 / 6.0;
    p = p * x + 0.5;
    p = p * x + 1.0;
    return p;
}

// ... and for |x| < 2^-5 the series cut after x^7: the first dropped term, x^8 / 9!, is below 2.6e-18 of phi there, far
// inside the rounding of the sum.  The trace kernel takes this form when EVERY live lane of the wave is that small (one
// ballot) -- most wave-steps: K ds is a few 1e-3 outside the hot spots of the exchange -- which takes 20 of the 34
// dependent fp64 operations out of the step's critical path.  The CPU checker always evaluates the long form; the two
// agree to the last bit or two, and the kernel is held to the checker at 1e-9.
__device__ __forceinline__ double phi_small(double x)
{
    // (fused multiply-adds: 7 operations for 14; the checker's unfused Horner form differs in the last bit or two)
    double p = 1.0 / 40320.0;
    p = __builtin_fma(p, x, 1.0 / 5040.0);
    p = __builtin_fma(p, x, 1.0 / 720.0);
    p = __builtin_fma(p, x, 1.0 / 120.0);
    p = __builtin_fma(p, x, 1.0 / 24.0);
    p = __builtin_fma(p, x, 1.0 / 6.0);
    p = __builtin_fma(p, x, 0.5);
    p = __builtin_fma(p, x, 1.0);
    return p;
}

// sqrt of a positive normal number far from the ends of the exponent range (a squared speed, cm^2/s^2), within an ulp:
// reciprocal-square-root estimate, one Goldschmidt step, two corrections -- without the range scaling and the special
// cases of the library sqrt (13 instructions for 27).  CBET extension only (the path length of a step); the reference
// path has no square root in its step.
__device__ __forceinline__ double sqrt_speed(double v2)
{
    const double r0 = __builtin_amdgcn_rsq(v2);
    double g = v2 * r0, h = 0.5 * r0;
    const double e = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, e, g); h = __builtin_fma(h, e, h);
    g = __builtin_fma(__builtin_fma(-g, g, v2), h, g);
    return __builtin_fma(__builtin_fma(-g, g, v2), h, g);
}

// ---- the CBET hook of a step: k_trace_window<., ., CBET >= 1> (the deposit passes) and ray_step<true, ., .> (the exit pass and
// the path recorder) both call the three functions below, so a ray's exit energy is what the deposition pass leaves it by construction
// The two factors of an axis are d = 1 - |o| and 1 - d (:329-336); which of them comes first is the lane's
// flip bit.  Without selects: F0 = +-(|o| - h), h = 1.0 with the sign flipped for a flipped lane (exactly
// d), h = 0.0 otherwise (|o| itself: the reference's 1 - (1 - |o|) up to 1.1e-16), F1 = 1 - F0 (exactly
// 1 - d, or exactly d).  Three instructions and one conversion per axis instead of six.
__device__ __forceinline__ void factor_pair(double o, int flip, double &f0, double &f1)
{
    const double g = fabs(o) - (double)flip;
    f0 = __hiloint2double(__double2hiint(g) ^ (flip << 31), __double2loint(g));
    f1 = 1.0 - f0;
}

// The clamped exponent K ds of a step: K at the lane's eight deposit nodes X0..Z1 (haloed) of gain grid gk, weighted like the deposit (factor_pair's
// F), times the path length ds.  The pairwise tree makes the sum independent of the corner order (the flips swap operands of commutative adds only).
template <bool IDX64>
__device__ __forceinline__ double gain_exponent(const TraceArgs &a, const double *gk, int X0, int X1, int Y0, int Y1, int Z0, int Z1, double Fx0,
                                                double Fx1, double Fy0, double Fy1, double Fz0, double Fz1, int sXh, int sYh, double ds)
{
    const int nX0 = __mul24(X0, sXh), nX1 = __mul24(X1, sXh), nY0 = __mul24(Y0, sYh), nY1 = __mul24(Y1, sYh);
    // The two z nodes of an (x, y) column are neighbours in memory: FOUR 16-byte gathers instead of eight 8-byte
    // ones.  The column sums take the z factors by node (lower, upper), so nothing depends on the lane's z flip;
    // the x and y flips swap operands of commutative adds.
    const bool z0_low = Z0 < Z1;
    const int zl = z0_low ? Z0 : Z1;
    const double fz_lo = z0_low ? Fz0 : Fz1, fz_hi = z0_low ? Fz1 : Fz0;
    const gain_pair_t c00 = gain_load2<IDX64>(a, gk, (unsigned)(nX0 + nY0 + zl)), c10 = gain_load2<IDX64>(a, gk, (unsigned)(nX1 + nY0 + zl));
    const gain_pair_t c01 = gain_load2<IDX64>(a, gk, (unsigned)(nX0 + nY1 + zl)), c11 = gain_load2<IDX64>(a, gk, (unsigned)(nX1 + nY1 + zl));
    // Fused multiply-adds, z then x then y: 14 operations for the 23 of the unfused pairwise tree the CPU checker
    // evaluates (a relative 1e-16 per term; the kernels are held to the checker at 1e-9).  The sum does not depend
    // on the corner order beyond that: the flips swap which of two products is the addend.
    const double q00 = __builtin_fma(fz_hi, c00.y, fz_lo * c00.x), q10 = __builtin_fma(fz_hi, c10.y, fz_lo * c10.x);
    const double q01 = __builtin_fma(fz_hi, c01.y, fz_lo * c01.x), q11 = __builtin_fma(fz_hi, c11.y, fz_lo * c11.x);
    const double r0 = __builtin_fma(Fx1, q10, Fx0 * q00), r1 = __builtin_fma(Fx1, q11, Fx0 * q01);
    const double ksum = __builtin_fma(Fy1, r1, Fy0 * r0);
    double x = ksum * ds;
    if (x > a.max_exponent) x = a.max_exponent;
    if (x < -a.max_exponent) x = -a.max_exponent;
    return x;
}

// phi(x) of the hook by the wave's vote (the caller's ballot, masked with ITS live lanes): phi_small when every live lane's |x| < kPhiSmallBelow
constexpr double kPhiSmallBelow = 0.03125;
__device__ __forceinline__ double gain_phi(double x, bool wave_is_small) { return wave_is_small ? phi_small(x) : phi_det(x); }

// ---- the step of the no-deposit integrators: k_trace_exit (the exit pass) and k_trace_path (the path recorder) both call
// ray_step below, so a ray's position, node, energy, step count and status are the same in both by construction
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

// What a lane's steps do not change, built once in front of the loop: the grid's sides, the haloed gain grid's strides, the
// shipped kernel's lane flips (cbet_trace_window.hip: which of an axis's two nodes the lane takes first, from the lane
// index) and the lane's gain grid (GAIN only).
struct StepFrame {
    int nx, ny, nz, sXh, sYh;
    int pfx, pfy, pfz;
    const double *gk;
};
__device__ __forceinline__ StepFrame step_frame(const TraceArgs &a, int lane, const double *gk)
{
    return StepFrame{a.nx, a.ny, a.nz, a.sXh, a.sYh, lane & 1, (lane >> 1) & 1, (lane >> 3) & 1, gk};
}
__device__ __forceinline__ unsigned node_of(const StepFrame &f, const Ray &s) { return (unsigned)((s.ci * f.ny + s.cj) * f.nz + s.ck); }

// One step of a wave (/root/reference/launch_ray_XZ.cu:268-356).  The call is wave-uniform -- the hook votes with a ballot --
// and only lanes with `alive` step: kick from `rec`, drift, nearest-node update, the new node `cell` and its record into
// `rec`; GAIN: the CBET hook of k_trace_window<16, ., 1> before the absorption, its energy added to `gained`; the absorption
// (absorbing mode only: checked on the host), ABSORBED: added to `absorbed`; the stop test against the six `planes`, which
// the caller chooses how to read.  Returns stop_test's bits, 0 for a ray that goes on and for a lane that did not step.
template <bool GAIN, bool IDX64, bool ABSORBED>
__device__ __forceinline__ int ray_step(const TraceArgs &a, const StepFrame &f, const double *planes, bool alive, Ray &s, StepRecord &rec,
                                        unsigned &cell, double &absorbed, double &gained)
{
    double x = 0.0;                                       // GAIN: the clamped exponent K ds of the step
    if (alive) {
        // :268-278 kick, drift, position in cell units
        s.vx -= rec.kx;
        s.vy -= rec.ky;
        s.vz -= rec.kz;
        double fx, fy, fz;
        drift(a, s, fx, fy, fz);
        // :282-292 nearest-node update
        s.ci = relocate_closed(s.ci, fx, f.nx);
        s.cj = relocate_closed(s.cj, fy, f.ny);
        s.ck = relocate_closed(s.ck, fz, f.nz);
        // :296-305 the absorption coefficient now, the kicks of the next step
        cell = node_of(f, s);
        rec = load_record<IDX64>(a, cell);
        if (GAIN) {
            // K at the eight deposit nodes with the deposit weights (:319-339)
            const double ox = (fx - (double)s.ci) - 0.5, oy = (fy - (double)s.cj) - 0.5, oz = (fz - (double)s.ck) - 0.5;
            const bool ngx = ox < 0, ngy = oy < 0, ngz = oz < 0;
            const int lx = s.ci + 1 - (ngx ? 1 : 0), ly = s.cj + 1 - (ngy ? 1 : 0), lz = s.ck + 1 - (ngz ? 1 : 0);
            const bool hx = ngx != (f.pfx != 0), hy = ngy != (f.pfy != 0), hz = ngz != (f.pfz != 0);
            const int X0 = lx + (hx ? 1 : 0), X1 = lx + (hx ? 0 : 1);
            const int Y0 = ly + (hy ? 1 : 0), Y1 = ly + (hy ? 0 : 1);
            const int Z0 = lz + (hz ? 1 : 0), Z1 = lz + (hz ? 0 : 1);
            double Fx0, Fx1, Fy0, Fy1, Fz0, Fz1;
            factor_pair(ox, f.pfx, Fx0, Fx1);
            factor_pair(oy, f.pfy, Fy0, Fy1);
            factor_pair(oz, f.pfz, Fz0, Fz1);
            const double ds = sqrt_speed(__builtin_fma(s.vz, s.vz, __builtin_fma(s.vy, s.vy, s.vx * s.vx))) * a.dt;
            x = gain_exponent<IDX64>(a, f.gk, X0, X1, Y0, Y1, Z0, Z1, Fx0, Fx1, Fy0, Fy1, Fz0, Fz1, f.sXh, f.sYh, ds);
        }
    }
    if (GAIN) {
        const bool small = __builtin_amdgcn_ballot_w64(alive && !(fabs(x) < kPhiSmallBelow)) == 0ull;
        if (alive) {
            const double phi = gain_phi(x, small);
            const double dg = s.uray * (x * phi);
            gained += dg;
            s.uray = s.uray + dg;
        }
    }
    int end = 0;
    if (alive) {
        const double inc = rec.kap * s.uray;              // :305-311
        s.uray -= inc;
        if (ABSORBED) absorbed += inc;
        end = stop_test(s, planes);                       // :351-356; the bits say which of its conditions held
    }
    return end;
}

// ... and their launch.  Wide (64-bit) indexing: forced, a step-record table beyond 2^32 bytes, or a gain grid of 2^32 bytes.
inline bool wide_index(const TraceArgs &a, bool force_idx64)
{
    return force_idx64 || sizeof(StepRecord) * (unsigned long long)a.nx * a.ny * a.nz > (1ull << 32) ||
           (a.gain && 8ull * (unsigned long long)a.hsize >= (1ull << 32));
}
// The GAIN x IDX64 instantiation a launch needs: launch(gain, wide) gets the two as std::bool_constant values and launches
// k<gain, wide> -- a generic lambda, since a kernel template cannot be passed by name.
template <class Launch>
hipError_t launch_gain_by_index(const TraceArgs &a, bool force_idx64, Launch launch)
{
    const bool wide = wide_index(a, force_idx64);
    if (a.gain) {
        if (wide) launch(std::true_type{}, std::true_type{});
        else launch(std::true_type{}, std::false_type{});
    } else {
        if (wide) launch(std::false_type{}, std::true_type{});
        else launch(std::false_type{}, std::false_type{});
    }
    return hipGetLastError();
}

// The work item of workgroup `w` of a launch: which (beam, patch) bundle.  The list is beam-major -- consecutive
// workgroups are neighbouring patches of one beam and share table lines in L2/MALL -- with each beam's patches
// longest rays first (a globally longest-first order and a patch-major order were measured 9-17 % slower).  A
// shard is a CONTIGUOUS 1/shard_count of that list (first_item .. first_item + count): a rank then walks ~7.5
// whole beams of the 60 and touches only their stretch of the 537 MB record table, where an interleaved split
// makes every rank touch every beam's (one rank's 1/8 share: 3.2 ms contiguous, 3.4 ms interleaved).
// (Round 3 measured the alternative of visiting a share in LENGTH CLASSES -- every beam's longest bundles first,
// beam by beam inside a class, so that a 1/8 share ends on short bundles: the launch's tail shrinks, but ~9 beams'
// stretches of the record table are then live at once instead of ~2 and the whole pass is 15-22 % slower; a 1/8
// share alone 3.45 ms against 3.32.  profiles/r3/experiments/length_class_order.log.)
__device__ __forceinline__ bool work_item(const TraceArgs &a, long w, int &beam, int &patch)
{
    const long g = a.first_item + w;
    if (w >= a.item_count) return false;  // wave-uniform
    const int beam_local = (int)(g / a.bundles_per_beam);
    patch = (int)(g - (long)beam_local * a.bundles_per_beam);
    beam = a.beam_lo + beam_local;
    return true;
}

}  // namespace cbet
#endif
