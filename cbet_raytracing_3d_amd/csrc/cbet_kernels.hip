// cbet_kernels.hip -- gfx950 (CDNA4) kernels of the ray-integrator path: the node-table kernel and the two
// cross-check formulations of the ray integrator.  The shipped integrator is cbet_trace_window.hip.
//
// Built with -ffp-contract=off: every per-ray fp64 operation below is the single IEEE operation the
// reference's statement performs (/root/reference/launch_ray_XZ.cu:117-359), in the same order, so
// a ray's trajectory, absorbed energy and the eight deposit values are the values the CPU oracle
// computes; only the order in which different rays' deposits are summed is free.
//
//   * k_tabulate     : the radial (r, ne, Te) profile is evaluated ONCE per node into two node
//                      tables in HBM, ne3d and kappa3d (= ed/ncrit*nuei*dt, launch_ray_XZ.cu:296-305
//                      without the trailing *uray).  The reference re-interpolates the profile eight
//                      times per ray-step (8 bisections + 9 sqrt + 9 div); with the tables a ray-step is
//                      seven 8-byte gathers and ~60 flops, no sqrt/div (k_trace_simple) -- or, folded once
//                      more into one 32-byte record per node by k_step_table, a single gather (the shipped kernel).
//   * k_plasma_records : both of the above in one pass (the plain pass's preparation): ne is evaluated per x-plane of a
//                      y-z tile into a three-plane LDS ring, and the records are formed from the ring instead of from
//                      the table k_tabulate has just written to HBM.  Bitwise the two-kernel path's tables and records.
//   * k_trace_simple : one wavefront = one 8x8-ray patch, the reference's step loop written plainly
//                      (literal relocation loop, no software pipeline), with the deposit either as
//       1  GLOBAL : 8 global_atomic_add_f64 per ray-step -- the reference's own scheme, the baseline; or
//       2  TAGGED : a wave-private toroidal LDS tile with node tags; slots are claimed by LDS CAS and
//                   written back with one global atomic when another node claims them.
//     Both exist to cross-check the shipped kernel (tests/) and to price its deposit scheme.
#include <hip/hip_runtime.h>

#include "cbet_node_kernel.h"
#include "cbet_node_model.h"
#include "cbet_trace_common.h"

namespace cbet {
namespace {

// One node's table entries, launch_ray_XZ.cu:296-305: ed = ne at the node's radius, kap = ed/ncrit*nuei*dt (the absorbed
// fraction up to the trailing "* uray").  Every statement is the reference's, in its order (cbet_node_model.h); both table
// kernels use it.
__device__ __forceinline__ void node_plasma(const TabulateArgs &a, const double *s_r, const double *s_ne, const double *s_te,
                                            int i, int j, int k, double &ed, double &kap)
{
    double sx, sy, sz, rho, etemp;
    node_centre(a, i, j, k, 0.0, 0.0, 0.0, sx, sy, sz, rho);       // :296
    interp2(s_ne, s_te, s_r, rho, a.nprofile, ed, etemp);           // :297-298
    kap = kappa(ed, etemp, a.ncrit, a.dt);                          // :299-305
}

// ---------------------------------------------------------------------------------------------
// Node tables.  One thread per node, grid-stride; the 3 x nprofile profile is staged in LDS
// (the one thing kept from the reference's layout, launch_ray_XZ.cu:136-150).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_tabulate(const TabulateArgs a)
{
    extern __shared__ double s_prof[];
    double *s_r = s_prof, *s_ne = s_prof + a.nprofile, *s_te = s_prof + 2 * a.nprofile;
    for (int i = threadIdx.x; i < a.nprofile; i += blockDim.x) {
        s_r[i] = a.r[i];
        s_ne[i] = a.ne[i];
        s_te[i] = a.te[i];
    }
    __syncthreads();
    const long total = (long)a.nx * a.ny * a.nz;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int k = (int)(idx % a.nz);
        const long ij = idx / a.nz;
        const int j = (int)(ij % a.ny);
        const int i = (int)(ij / a.ny);
        double ed, kap;
        node_plasma(a, s_r, s_ne, s_te, i, j, k, ed, kap);
        a.ne3d[idx] = ed;
        a.kap3d[idx] = kap;
    }
}

// ---------------------------------------------------------------------------------------------
// Step records (cbet_device.h StepRecord): one thread per node, z fastest.  Bound: HBM, 16 B read (plus
// neighbour lines from cache) and 32 B written per node.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_step_table(const StepTableArgs a)
{
    const long total = (long)a.nx * a.ny * a.nz;
    const long stride = (long)gridDim.x * blockDim.x;
    const long sY = a.nz, sX = (long)a.ny * a.nz;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int k = (int)(idx % a.nz);
        const long ij = idx / a.nz;
        const int j = (int)(ij % a.ny);
        const int i = (int)(ij / a.ny);
        long oxm, oxp, oym, oyp, ozm, ozp;                           // :212-238
        face_pair(i, a.nx, oxm, oxp, sX);
        face_pair(j, a.ny, oym, oyp, sY);
        face_pair(k, a.nz, ozm, ozp);
        StepRecord r;
        r.kx = a.xconst * (a.ne3d[idx + oxp] - a.ne3d[idx + oxm]);   // :268
        r.ky = a.yconst * (a.ne3d[idx + oyp] - a.ne3d[idx + oym]);   // :269
        r.kz = a.zconst * (a.ne3d[idx + ozp] - a.ne3d[idx + ozm]);   // :270
        r.kap = a.kap3d[idx];
        a.rec[idx] = r;
    }
}

// ---------------------------------------------------------------------------------------------
// Node tables AND step records in one pass (the preparation of a plain pass: k_tabulate + k_step_table without the
// trip of ne3d through HBM in between).
//
// A workgroup owns a tile of kPrTY x kPrTZ nodes in (y, z) and marches over kPrXC x-planes.  Per plane p it evaluates
// node_plasma for the tile's nodes (and, for planes of its own chunk, ne alone for the one-node cross halo in y and z)
// into slot p % 3 of a three-plane LDS ring, writes ne3d / kappa3d for its own nodes, and -- as soon as the plane on
// the far side of a node is in the ring -- forms the node's record from LDS with k_step_table's operands:
// c * (ne(+1) - ne(-1)), one-sided on the faces (launch_ray_XZ.cu:212-226, 268-270: face_pair).
// Tiles are CLAMPED into the grid (a partial last tile overlaps its neighbour and writes the same values again), so a
// face node's one-sided pair (n-3, n-1) always lies in its own tile; planes 0 and nx-1 are emitted together with their
// neighbours (at p = 2 and p = nx-1), when the ring holds both planes of their pair.
// Stores: ne3d / kappa3d 8 B per lane along z; records 16 B per lane along z -- lane pair (2m, 2m+1) writes the
// {kx, ky} and {kz, kap} halves of node m, a wave 1 KB of whole lines.
// Work repeated for the halo: (kPrXC + 2) / kPrXC tile planes and 2 (kPrTY + kPrTZ) halo nodes per kPrTY kPrTZ tile
// nodes of ne alone = 1.41 ne evaluations per node (1 kappa); LDS 28,128 B + the profile (38,760 B at 443 rows:
// four workgroups = 16 waves per CU).  DESIGN.md 4.1.
// ---------------------------------------------------------------------------------------------
constexpr int kPrTY = 8, kPrTZ = 64, kPrXC = 16, kPrThreads = 256;
constexpr int kPrPZ = kPrTZ + 2;                          // ring row pitch (doubles): the tile's row and its two halo nodes
constexpr int kPrPlane = (kPrTY + 2) * kPrPZ;             // one ring plane
constexpr int kPrTile = kPrTY * kPrTZ;
constexpr int kPrItems = kPrTile + 2 * kPrTZ + 2 * kPrTY; // tile nodes, then the y halo rows, then the z halo columns

__global__ void __launch_bounds__(kPrThreads) k_plasma_records(const PlasmaRecordsArgs a)
{
    extern __shared__ double s_prof[];
    const TabulateArgs &t = a.t;
    double *s_r = s_prof, *s_ne = s_prof + t.nprofile, *s_te = s_prof + 2 * t.nprofile;
    double *s_ring = s_prof + 3 * t.nprofile;             // [3][kPrTY + 2][kPrPZ] ne
    double *s_kap = s_ring + 3 * kPrPlane;                // [3][kPrTile] kappa of the tile's own nodes
    const int tid = threadIdx.x;
    for (int i = tid; i < t.nprofile; i += kPrThreads) {
        s_r[i] = t.r[i];
        s_ne[i] = t.ne[i];
        s_te[i] = t.te[i];
    }
    __syncthreads();
    const int nx = t.nx, ny = t.ny, nz = t.nz;
    const int k0 = max(0, min((int)blockIdx.x * kPrTZ, nz - kPrTZ));
    const int j0 = max(0, min((int)blockIdx.y * kPrTY, ny - kPrTY));
    const int x0 = (int)blockIdx.z * kPrXC, x1 = min(x0 + kPrXC, nx);
    // planes the chunk's records need: its own and one beyond each end, (0, 2) / (nx-3, nx-1) at the faces
    const int pa = x0 == 0 ? 0 : min(x0 - 1, nx - 3);
    const int pb = x1 == nx ? nx : max(x1 + 1, 3);

    // records of plane i from the ring: x pair in planes xl / xh, y and z pairs in plane i itself
    auto emit = [&](int i, int xl, int xh) {
        const double *lo = s_ring + (xl % 3) * kPrPlane, *hi = s_ring + (xh % 3) * kPrPlane, *mid = s_ring + (i % 3) * kPrPlane;
        const double *kap = s_kap + (i % 3) * kPrTile;
        for (int q = tid; q < 2 * kPrTile; q += kPrThreads) {
            const int n = q >> 1, jr = n / kPrTZ, kr = n % kPrTZ;
            const int j = j0 + jr, k = k0 + kr;
            if (j >= ny || k >= nz) continue;
            const int c = (jr + 1) * kPrPZ + kr + 1;
            double v0, v1;
            int m, p;
            if ((q & 1) == 0) {
                face_pair(j, ny, m, p);
                v0 = a.xconst * (hi[c] - lo[c]);                                 // :268
                v1 = a.yconst * (mid[c + p * kPrPZ] - mid[c + m * kPrPZ]);       // :269
            } else {
                face_pair(k, nz, m, p);
                v0 = a.zconst * (mid[c + p] - mid[c + m]);                       // :270
                v1 = kap[n];
            }
            const long idx = ((long)i * ny + j) * nz + k;
            reinterpret_cast<double2 *>(a.rec + idx)[q & 1] = make_double2(v0, v1);
        }
    };

    for (int p = pa; p < pb; ++p) {
        const bool own_plane = p >= x0 && p < x1;
        double *ring = s_ring + (p % 3) * kPrPlane;
        for (int n = tid; n < (own_plane ? kPrItems : kPrTile); n += kPrThreads) {
            int jj, kk;
            if (n < kPrTile) {
                jj = 1 + n / kPrTZ; kk = 1 + n % kPrTZ;
            } else if (n < kPrTile + 2 * kPrTZ) {
                const int h = n - kPrTile;
                jj = h < kPrTZ ? 0 : kPrTY + 1; kk = 1 + h % kPrTZ;
            } else {
                const int h = n - kPrTile - 2 * kPrTZ;
                kk = h < kPrTY ? 0 : kPrTZ + 1; jj = 1 + h % kPrTY;
            }
            const int j = j0 + jj - 1, k = k0 + kk - 1;
            if (j < 0 || j >= ny || k < 0 || k >= nz) continue;
            double ed, kap;
            if (own_plane && n < kPrTile) {
                node_plasma(t, s_r, s_ne, s_te, p, j, k, ed, kap);
                s_kap[(p % 3) * kPrTile + n] = kap;
                const long idx = ((long)p * ny + j) * nz + k;
                t.ne3d[idx] = ed;
                t.kap3d[idx] = kap;
            } else {
                node_plasma(t, s_r, s_ne, s_te, p, j, k, ed, kap);     // halo: ne alone (kap is dead code here)
            }
            ring[jj * kPrPZ + kk] = ed;
        }
        __syncthreads();
        if (p == 2 && x0 == 0) emit(0, 0, 2);
        if (p - 1 >= 1 && p - 1 >= x0 && p - 1 < x1) emit(p - 1, p - 2, p);
        if (p == nx - 1 && x1 == nx) emit(nx - 1, nx - 3, nx - 1);
        __syncthreads();            // the next plane overwrites the slot of plane p - 2
    }
}

// ---------------------------------------------------------------------------------------------
// Wave-private LDS write-combining window for the deposits.
//
// slot(i,j,k) = the node's haloed indices taken modulo W per axis (a W^3 torus), tag = the node's
// flat haloed index.  All 64 lanes of the wave run this in lock step (one wave per workgroup, so
// no other wave touches the window); LDS operations of one wave execute in program order.
//   fast path : read the 8 tags; where tag == node, ds_add_f64 the weight.
//   slow path : per corner, retry until done, each round in two ordered phases: (1) re-read the
//               tag, lanes that match add; (2) the rest CAS the tag to their node -- exactly one
//               lane per slot wins, swaps its weight in as the new accumulator value and writes
//               the old (tag, sum) back to HBM with one atomic.
// Invariant: an add under tag T is always issued before the instruction that replaces T, so a
// swapped-out sum holds every add made under the old tag and nothing else.
// ---------------------------------------------------------------------------------------------
template <int WL>
struct LdsWindow {
    static constexpr int W = 1 << WL;
    static constexpr int NSLOT = W * W * W;
    double *val;
    unsigned *tag;
    const TraceArgs *args;

    __device__ __forceinline__ unsigned slot(int i, int j, int k) const
    {
        return (unsigned)((((i & (W - 1)) << WL) | (j & (W - 1))) << WL | (k & (W - 1)));
    }
    __device__ __forceinline__ void clear(int lane)
    {
        for (int s = lane; s < NSLOT; s += kWave) {
            val[s] = 0.0;
            tag[s] = kEmptyTag;
        }
    }
    __device__ __forceinline__ void add(unsigned s, double w)
    {
        if (CBET_AUDIT(*args, s < (unsigned)NSLOT))
            __hip_atomic_fetch_add(&val[s], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // Write every live slot back (wave end).
    __device__ __forceinline__ int flush(int lane, double *edep)
    {
        int n = 0;
        for (int s = lane; s < NSLOT; s += kWave) {
            const unsigned t = tag[s];
            if (t != kEmptyTag) {
                global_add(*args, &edep[t], val[s]);
                ++n;
            }
        }
        return n;
    }
};

template <int WL>
__device__ __forceinline__ void lds_deposit8(LdsWindow<WL> &win, bool pending, const unsigned (&slot)[8],
                                             const unsigned (&node)[8], const double (&w)[8],
                                             double *edep, int &n_evict)
{
    unsigned miss = 0;
    if (pending) {
        unsigned t[8];
#pragma unroll
        for (int c = 0; c < 8; ++c)
            t[c] = __hip_atomic_load(&win.tag[slot[c]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (t[c] == node[c])
                win.add(slot[c], w[c]);
            else
                miss |= 1u << c;
        }
    }
    if (!__any(miss != 0)) return;
    __builtin_amdgcn_wave_barrier();  // every fast-path add is issued before any slot changes owner
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        bool pend = (miss >> c) & 1u;
        while (__any(pend)) {
            unsigned t = 0;
            if (pend)
                t = __hip_atomic_load(&win.tag[slot[c]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            // phase 1: lanes whose node owns the slot add.  This must complete, for ALL lanes,
            // before phase 2 lets any lane hand the slot to another node -- hence two separate
            // statements with a wave barrier between them, not an if/else whose block order the
            // compiler chooses.
            if (pend && t == node[c]) {
                win.add(slot[c], w[c]);
                pend = false;
            }
            __builtin_amdgcn_wave_barrier();
            // phase 2: the others try to claim the slot; one lane per slot wins the CAS, swaps its
            // weight in as the new sum and writes the previous owner's sum back to HBM.  Losers
            // (and lanes whose node just became the owner) go round again.
            if (pend) {
                unsigned expect = t;
                const bool won = __hip_atomic_compare_exchange_strong(
                    &win.tag[slot[c]], &expect, node[c], __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                    __HIP_MEMORY_SCOPE_WORKGROUP);
                if (won) {
                    const unsigned long long old = __hip_atomic_exchange(
                        reinterpret_cast<unsigned long long *>(&win.val[slot[c]]),
                        (unsigned long long)__double_as_longlong(w[c]), __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (t != kEmptyTag) {
                        global_add(*win.args, &edep[t], __longlong_as_double((long long)old));
                        ++n_evict;
                    }
                    pend = false;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The cross-check integrator.  DEPOSIT 1: 8 global atomics per step; 2: tagged 8^3 LDS window.
// Absorption (def.cuh:118) and the table index width are run-time here: nothing in it is tuned.
// ---------------------------------------------------------------------------------------------
template <int DEPOSIT>
__global__ void __launch_bounds__(kWave) k_trace_simple(const TraceArgs a)
{
    constexpr int WL = 3;
    constexpr int NSLOT = DEPOSIT == 2 ? (1 << (3 * WL)) : 1;
    __shared__ double s_val[NSLOT];
    __shared__ unsigned s_tag[NSLOT];
    const int lane = threadIdx.x;
    int beam, patch;
    if (!work_item(a, blockIdx.x, beam, patch)) return;
    double *const edep = a.edep + (long)(beam - a.grid_beam0) * a.grid_stride;
    const bool absorb = a.absorption == 1;

    Ray s;
    int li;
    const bool launched = launch_lane(a, beam, patch, lane, s, li);
    bool alive = launched;

    const int nx = a.nx, ny = a.ny, nz = a.nz;
    const long sY = nz, sX = (long)ny * nz;                       // node-table strides (elements)
    const int sYh = a.sYh, sXh = a.sXh;                           // haloed edep strides (:5-7)
    int nsteps = 0, n_atomics = 0, n_evict = 0;
    unsigned wave_steps = 0;

    LdsWindow<WL> tagged{s_val, s_tag, &a};
    if (DEPOSIT == 2) {
        tagged.clear(lane);
        __syncthreads();
    }

    for (int tt = 0; tt < a.nt; ++tt) {                        // :207
        if (__ballot(alive) == 0) break;
        ++wave_steps;
        unsigned slot[8] = {0, 0, 0, 0, 0, 0, 0, 0}, node[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        double wgt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (alive) {
            int im, ip, jm, jp, km, kp;                            // :212-238 neighbours of the current node, as offsets from it
            face_pair(s.ci, nx, im, ip);
            face_pair(s.cj, ny, jm, jp);
            face_pair(s.ck, nz, km, kp);
            auto ne_at = [&](int i, int j, int k) { return node_load<true>(a, a.ne3d, (unsigned)(i * sX + j * sY + k), a.audit_nodes); };
            // :254-278 six gathers, kick, drift, position in cell units
            s.vx -= a.xconst * (ne_at(s.ci + ip, s.cj, s.ck) - ne_at(s.ci + im, s.cj, s.ck));
            s.vy -= a.yconst * (ne_at(s.ci, s.cj + jp, s.ck) - ne_at(s.ci, s.cj + jm, s.ck));
            s.vz -= a.zconst * (ne_at(s.ci, s.cj, s.ck + kp) - ne_at(s.ci, s.cj, s.ck + km));
            double fx, fy, fz;
            drift(a, s, fx, fy, fz);
            // :282-292 nearest-node update (the literal loop)
            s.ci = relocate_loop(s.ci, fx, nx);
            s.cj = relocate_loop(s.cj, fy, ny);
            s.ck = relocate_loop(s.ck, fz, nz);
            // :296-311 absorbed energy
            double inc;
            if (absorb) {
                inc = node_load<true>(a, a.kap3d, (unsigned)(s.ci * sX + s.cj * sY + s.ck), a.audit_nodes) * s.uray;
                s.uray -= inc;
            } else {
                inc = s.uray;
            }
            // :319-339 weights, in the reference's corner order
            const double ox = fx - s.ci - 0.5, oy = fy - s.cj - 0.5, oz = fz - s.ck - 0.5;
            const double dm = 1.0 - fabs(ox), dn = 1.0 - fabs(oy), dl = 1.0 - fabs(oz);
            const int X0 = s.ci + 1, X1 = X0 + (ox < 0 ? -1 : 1);
            const int Y0 = s.cj + 1, Y1 = Y0 + (oy < 0 ? -1 : 1);
            const int Z0 = s.ck + 1, Z1 = Z0 + (oz < 0 ? -1 : 1);
            const double Fx0 = 1.0 - dm, Fy0 = 1.0 - dn, Fz0 = 1.0 - dl;
            const double zy00 = Fz0 * Fy0, zy10 = dl * Fy0, zy01 = Fz0 * dn, zy11 = dl * dn;
            wgt[0] = zy00 * Fx0 * inc; wgt[1] = zy00 * dm * inc; wgt[2] = zy10 * Fx0 * inc; wgt[3] = zy10 * dm * inc;
            wgt[4] = zy01 * Fx0 * inc; wgt[5] = zy01 * dm * inc; wgt[6] = zy11 * Fx0 * inc; wgt[7] = zy11 * dm * inc;
            const int nX0 = X0 * sXh, nX1 = X1 * sXh, nY0 = Y0 * sYh, nY1 = Y1 * sYh;
            node[0] = nX0 + nY0 + Z0; node[1] = nX1 + nY0 + Z0; node[2] = nX0 + nY0 + Z1; node[3] = nX1 + nY0 + Z1;
            node[4] = nX0 + nY1 + Z0; node[5] = nX1 + nY1 + Z0; node[6] = nX0 + nY1 + Z1; node[7] = nX1 + nY1 + Z1;
            if (DEPOSIT == 1) {
#pragma unroll
                for (int c = 0; c < 8; ++c) global_add(a, &edep[node[c]], wgt[c]);   // :341-348
                n_atomics += 8;
            } else {
                slot[0] = tagged.slot(X0, Y0, Z0); slot[1] = tagged.slot(X1, Y0, Z0);
                slot[2] = tagged.slot(X0, Y0, Z1); slot[3] = tagged.slot(X1, Y0, Z1);
                slot[4] = tagged.slot(X0, Y1, Z0); slot[5] = tagged.slot(X1, Y1, Z0);
                slot[6] = tagged.slot(X0, Y1, Z1); slot[7] = tagged.slot(X1, Y1, Z1);
            }
            ++nsteps;
        }
        if (DEPOSIT == 2) lds_deposit8<WL>(tagged, alive, slot, node, wgt, edep, n_evict);
        if (alive && stop_test(s, a.bounds) != 0) alive = false;   // :351-356
    }
    if (DEPOSIT == 2) {
        __syncthreads();
        n_atomics += tagged.flush(lane, edep) + n_evict;
    }
    count_steps_and_rays(a, lane, nsteps, launched);
    const int tot_at = wave_sum(n_atomics), tot_ev = wave_sum(n_evict);
    if (lane == 0) {
        atomicAdd(&a.counters[kCntGlobalAtomics], (unsigned long long)tot_at);
        atomicAdd(&a.counters[kCntEvictions], (unsigned long long)tot_ev);
        atomicAdd(&a.counters[kCntWaveSteps], (unsigned long long)wave_steps);
    }
}

#ifdef CBET_DEBUG_BOUNDS
__device__ unsigned long long g_audit_violations;
#endif

}  // namespace

hipError_t launch_tabulate(const TabulateArgs &a, hipStream_t stream)
{
    const size_t lds = sizeof(double) * 3 * (size_t)a.nprofile;
    hipLaunchKernelGGL(k_tabulate, dim3(node_blocks((long)a.nx * a.ny * a.nz)), dim3(256), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_step_table(const StepTableArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(k_step_table, dim3(node_blocks((long)a.nx * a.ny * a.nz)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

size_t plasma_records_lds(int nprofile)
{
    return sizeof(double) * (3 * (size_t)nprofile + 3 * (size_t)kPrPlane + 3 * (size_t)kPrTile);
}

hipError_t launch_plasma_records(const PlasmaRecordsArgs &a, hipStream_t stream)
{
    const dim3 grid((unsigned)((a.t.nz + kPrTZ - 1) / kPrTZ), (unsigned)((a.t.ny + kPrTY - 1) / kPrTY),
                    (unsigned)((a.t.nx + kPrXC - 1) / kPrXC));
    hipLaunchKernelGGL(k_plasma_records, grid, dim3(kPrThreads), plasma_records_lds(a.t.nprofile), stream, a);
    return hipGetLastError();
}

hipError_t audit_violations(unsigned long long *out, bool reset, hipStream_t stream)
{
#ifdef CBET_DEBUG_BOUNDS
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_audit_violations), sizeof *out);
    if (e == hipSuccess && reset) {
        const unsigned long long zero = 0;
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_audit_violations), &zero, sizeof zero);
    }
    return e;
#else
    (void)out; (void)reset; (void)stream;
    return hipErrorNotSupported;
#endif
}

hipError_t launch_trace(const TraceArgs &a0, int variant, bool force_idx64, hipStream_t stream, const PathArgs *path,
                        const SbsArgs *sbs, const GainArgs *sbs_gain)
{
    TraceArgs a = a0;
#ifdef CBET_DEBUG_BOUNDS
    {   // the ranges the audited accesses are checked against
        const long cells = (long)(a.nx + 2) * a.sXh;
        a.audit_lo = a.edep;
        a.audit_hi = a.edep + (a.grid_stride ? a.grid_stride * (long)(a.beam_lo - a.grid_beam0 + a.nbeams_local) : cells);
        if (a.quantity != 0) a.audit_hi = a.edep + 4 * a.comp_stride;   // the field pass writes four component arrays
        a.audit_nodes = (unsigned long long)a.nx * a.ny * a.nz;
        a.audit_hsize = (unsigned long long)a.hsize;
        hipError_t e = hipGetSymbolAddress((void **)&a.audit_count, HIP_SYMBOL(g_audit_violations));
        if (e != hipSuccess) return e;
    }
#endif
    if (variant == CBET_KERNEL_LDS_WINDOW) return launch_trace_window(a, force_idx64, stream);
    if (variant == kTraceExits) return launch_trace_exit(a, force_idx64, stream);
    if (variant == kTracePaths) return path ? launch_trace_path(a, *path, force_idx64, stream) : hipErrorInvalidValue;
    if (variant == kTraceBackscatter)
        return sbs && sbs_gain ? launch_trace_backscatter(a, *sbs_gain, *sbs, force_idx64, stream) : hipErrorInvalidValue;
    const long waves = a.item_count;
    if (waves <= 0) return hipSuccess;
    const dim3 grid((unsigned)waves);
    if (variant == CBET_KERNEL_GLOBAL_ATOMICS) hipLaunchKernelGGL((k_trace_simple<1>), grid, dim3(kWave), 0, stream, a);
    else hipLaunchKernelGGL((k_trace_simple<2>), grid, dim3(kWave), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cbet
