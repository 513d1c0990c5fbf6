// cbet_sph_modes.hip -- spherical-harmonic mode spectra of deposit grids on shells.
//
// a[g][s][c] = sum over the nodes of shell s of E_g(node) Y_c(node), with the real orthonormal harmonics of
// include/cbet_mi355x.h.  One block per (m-group, shell, chunk of G grids):
//   - m-groups: group 0 holds m = 0 (l = 0 .. lmax); group k >= 1 holds m = k (l = k .. lmax) and, when it is larger,
//     m = lmax + 1 - k (l = lmax + 1 - k .. lmax): at most lmax + 1 (l, m) slots per group, each with a cos and a sin
//     accumulator, so a thread's accumulators are registers indexed by the unrolled slot number;
//   - the block enumerates only the nodes that can lie in its shell: for every (I, J) row inside the shell's bounding
//     square, the one or two K segments where the row crosses the shell (with a node of margin).  The candidates are
//     tested with the exact node radius and the members are compacted into a queue in LDS, so every batch of the
//     harmonic work runs with all lanes busy;
//   - Y comes from the normalised recurrence: Y_mm by the product of sqrt((2k+1)/2k) sin(theta), then
//     Y_lm = a_lm (cos(theta) Y_{l-1,m} - b_lm Y_{l-2,m}); cos(m phi) and sin(m phi) are powers of (x + iy) / rho;
//   - the block sums its threads' accumulators in a fixed tree (no atomics), so the result is the same bits from run to
//     run, and the order depends on logical node indices only (a padded grid gives the dense grid's bits).
// Every (g, s, c) output is written by exactly one block.
#include <hip/hip_runtime.h>

#include <cmath>

#include "cbet_device.h"

namespace cbet {
namespace {

// The nodes N of one axis whose offset (N - 1) d + mn - c from the centre can lie in [lo, hi]: [N0, N1] (one node of
// margin each side), clamped to the haloed range [0, n + 1].  Empty when N0 > N1.
__device__ __forceinline__ void node_range(double lo, double hi, double c, double mn, double d, int n, int &N0, int &N1)
{
    double u0 = (lo + c - mn) / d, u1 = (hi + c - mn) / d;
    u0 = fmin(fmax(u0, -4.0), n + 4.0);
    u1 = fmin(fmax(u1, -4.0), n + 4.0);
    N0 = max(0, (int)floor(u0));          // (floor(u0) - 1) + 1
    N1 = min(n + 1, (int)ceil(u1) + 2);   // (ceil(u1) + 1) + 1
}

// Exclusive prefix sum of v over the block of NT threads; *total = the block's sum.  Integer: exact.
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int *s_wtot, int *total)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    __syncthreads();                       // the previous scan's readers are done with s_wtot
    if (lane == kWave - 1) s_wtot[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NT / kWave; ++w) {
        const int t = s_wtot[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return before + inc - v;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);   // a + b on one lane, b + a on its partner: same bits
    return v;
}

template <int LMAX_T, int G, int NT>
__global__ void __launch_bounds__(NT) k_sph_modes(const SphArgs a)
{
    constexpr int kSphThreads = NT, kSphWaves = NT / kWave;
    constexpr int kSlots = LMAX_T + 1;
    constexpr int kNv = 2 * kSlots * G + G;            // cos / sin accumulators, then the shell energies
    __shared__ double s_ca[kSlots], s_cb[kSlots];      // a_lm, b_lm of each slot
    __shared__ double s_d[kSlots];                     // sqrt((2k + 1) / 2k)
    __shared__ int s_pref[kSphThreads];
    __shared__ int s_row[kSphThreads][4];              // I, J, first K of segment 1, its length
    __shared__ int s_k2[kSphThreads];                  // first K of segment 2
    __shared__ int s_queue[2 * kSphThreads];
    __shared__ int s_wtot[kSphWaves];
    __shared__ double s_red[kSphWaves][kNv];
    __shared__ int s_cnt[kSphWaves];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int group = blockIdx.x;
    const int s = a.nshell - 1 - (int)blockIdx.y;      // the outer (larger) shells are dispatched first
    const int g0 = (int)blockIdx.z * G;
    const int lmax = a.lmax;
    int ma, mb, na;                                    // slot j < na: m = ma, l = ma + j; else m = mb, l = mb + j - na
    if (group == 0) {
        ma = 0; na = lmax + 1; mb = -1;
    } else {
        ma = group; na = lmax + 1 - group; mb = lmax + 1 - group;
        if (mb <= ma) mb = -1;
    }
    const int nslots = mb < 0 ? na : lmax + 1;
    if (tid < nslots) {
        const int m = tid < na ? ma : mb, l = tid < na ? ma + tid : mb + tid - na;
        s_ca[tid] = l > m ? sqrt((double)(4 * l * l - 1) / (double)(l * l - m * m)) : 0.0;
        s_cb[tid] = l > m ? sqrt((double)((l - 1) * (l - 1) - m * m) / (double)(4 * (l - 1) * (l - 1) - 1)) : 0.0;
    }
    if (tid >= 1 && tid <= LMAX_T) s_d[tid] = sqrt((double)(2 * tid + 1) / (double)(2 * tid));

    const double r0 = a.r_edges[s], r1 = a.r_edges[s + 1];
    const double R1 = r1 * (1.0 + 1e-12), R0 = r0 * (1.0 - 1e-12);   // candidate bounds, wider than the exact test
    const long plane = (long)(a.ny + 2) * a.row_pitch;
    const double y00 = 1.0 / sqrt(4.0 * M_PI);
    const double sqrt2 = sqrt(2.0);

    double accC[kSlots][G], accS[kSlots][G], accE[G];
#pragma unroll
    for (int j = 0; j < kSlots; ++j)
#pragma unroll
        for (int g = 0; g < G; ++g) accC[j][g] = accS[j][g] = 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g) accE[g] = 0.0;
    int count = 0;

    // one member node (logical index (I (ny+2) + J) (nz+2) + K), or -1: an idle lane
    auto process = [&](int node) __attribute__((always_inline)) {
        const bool real = node >= 0;
        int I = 0, J = 0, K = 0;
        if (real) {
            const int hyz = (a.ny + 2) * (a.nz + 2);
            I = node / hyz;
            const int rem = node - I * hyz;
            J = rem / (a.nz + 2);
            K = rem - J * (a.nz + 2);
        }
        const double x = ((I - 1) * a.dx + a.xmin) - a.cx;
        const double y = ((J - 1) * a.dy + a.ymin) - a.cy;
        const double z = ((K - 1) * a.dz + a.zmin) - a.cz;
        const double r = sqrt(x * x + y * y + z * z);
        double ct = 0.0, st = 0.0, c1 = 1.0, s1 = 0.0, hi = 0.0;
        if (real && r > 0.0) {
            const double rho = sqrt(x * x + y * y);
            ct = z / r;
            st = rho / r;
            if (rho > 0.0) { c1 = x / rho; s1 = y / rho; }
            hi = 1.0;
        }
        double e[G], eh[G];                            // E, and E for l >= 1 (0 at r = 0)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            double v = 0.0;
            if (real && g0 + g < a.ngrids)
                v = a.edep ? a.edep[(long)(g0 + g) * a.grid_stride + (long)I * plane + (long)J * a.row_pitch + K] : 1.0;
            e[g] = v;
            eh[g] = v * hi;
            accE[g] += v;
        }
        count += real ? 1 : 0;
        // Y_mm and sqrt(2) cos / sin (m phi) of the group's m values
        double pa = y00, pb = 0.0, ca = 1.0, sa = 0.0, cb = 0.0, sb = 0.0;
        {
            double p = y00, cr = 1.0, si = 0.0;
            const int mtop = mb >= 0 ? mb : ma;
            for (int k = 1; k <= mtop; ++k) {
                p = (p * s_d[k]) * st;
                const double cn = cr * c1 - si * s1;
                si = cr * s1 + si * c1;
                cr = cn;
                if (k == ma) { pa = p; ca = sqrt2 * cr; sa = sqrt2 * si; }
                if (k == mb) { pb = p; cb = sqrt2 * cr; sb = sqrt2 * si; }
            }
        }
        double p1 = 0.0, p2 = 0.0, cm = ca, sm = sa;
#pragma unroll
        for (int j = 0; j < kSlots; ++j) {
            if (j < nslots) {
                double yv;
                if (j == 0) {
                    yv = pa; p1 = pa; p2 = 0.0;
                } else if (j == na) {
                    yv = pb; p1 = pb; p2 = 0.0; cm = cb; sm = sb;
                } else {
                    yv = s_ca[j] * fma(ct, p1, -(s_cb[j] * p2));
                    p2 = p1;
                    p1 = yv;
                }
                const double yc = yv * cm, ys = yv * sm;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const double w = j == 0 ? e[g] : eh[g];
                    accC[j][g] = fma(w, yc, accC[j][g]);
                    accS[j][g] = fma(w, ys, accS[j][g]);
                }
            }
        }
    };

    // the nodes that can lie in the shell: rows (I, J) of its bounding square, K segments per row
    int I0, I1, J0, J1;
    node_range(-R1, R1, a.cx, a.xmin, a.dx, a.nx, I0, I1);
    node_range(-R1, R1, a.cy, a.ymin, a.dy, a.ny, J0, J1);
    const int nJ = J1 - J0 + 1;
    const int nrows = (I1 >= I0 && nJ > 0) ? (I1 - I0 + 1) * nJ : 0;
    int qn = 0;                                        // members queued (the same in every thread)
    __syncthreads();                                   // the slot tables
    for (int row0 = 0; row0 < nrows; row0 += kSphThreads) {
        const int ri = row0 + tid;
        int I = 0, J = 0, k1 = 0, n1 = 0, k2 = 0, n2 = 0;
        if (ri < nrows) {
            I = I0 + ri / nJ;
            J = J0 + ri % nJ;
            const double x = ((I - 1) * a.dx + a.xmin) - a.cx;
            const double y = ((J - 1) * a.dy + a.ymin) - a.cy;
            const double q = x * x + y * y;
            const double h1sq = R1 * R1 - q;
            if (h1sq >= 0.0) {
                const double h1 = sqrt(h1sq), h0sq = R0 * R0 - q;
                int a0, a1;
                if (h0sq > 0.0) {
                    const double h0 = sqrt(h0sq);
                    int b0, b1;
                    node_range(-h1, -h0, a.cz, a.zmin, a.dz, a.nz, a0, a1);
                    node_range(h0, h1, a.cz, a.zmin, a.dz, a.nz, b0, b1);
                    if (a1 >= a0 && b1 >= b0 && a1 >= b0 - 1) {      // the segments touch: one
                        a1 = max(a1, b1);
                        b1 = b0 - 1;
                    }
                    k1 = a0; n1 = max(0, a1 - a0 + 1);
                    k2 = b0; n2 = max(0, b1 - b0 + 1);
                } else {
                    node_range(-h1, h1, a.cz, a.zmin, a.dz, a.nz, a0, a1);
                    k1 = a0; n1 = max(0, a1 - a0 + 1);
                }
            }
        }
        int total;
        const int pref = block_excl_scan<NT>(n1 + n2, s_wtot, &total);
        s_pref[tid] = pref;
        s_row[tid][0] = I; s_row[tid][1] = J; s_row[tid][2] = k1; s_row[tid][3] = n1;
        s_k2[tid] = k2;
        __syncthreads();
        for (int c0 = 0; c0 < total; c0 += kSphThreads) {
            const int t = c0 + tid;
            int node = -1;
            if (t < total) {
                int lo = 0, hi = kSphThreads - 1;                 // the last row whose prefix is <= t
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (s_pref[mid] <= t) lo = mid; else hi = mid - 1;
                }
                const int o = t - s_pref[lo];
                const int RI = s_row[lo][0], RJ = s_row[lo][1];
                const int K = o < s_row[lo][3] ? s_row[lo][2] + o : s_k2[lo] + (o - s_row[lo][3]);
                const double x = ((RI - 1) * a.dx + a.xmin) - a.cx;
                const double y = ((RJ - 1) * a.dy + a.ymin) - a.cy;
                const double z = ((K - 1) * a.dz + a.zmin) - a.cz;
                const double r = sqrt(x * x + y * y + z * z);
                if (r0 <= r && r < r1) node = (RI * (a.ny + 2) + RJ) * (a.nz + 2) + K;
            }
            int mtot;
            const int mpos = block_excl_scan<NT>(node >= 0 ? 1 : 0, s_wtot, &mtot);
            if (node >= 0) s_queue[qn + mpos] = node;
            __syncthreads();
            qn += mtot;
            if (qn >= kSphThreads) {
                process(s_queue[tid]);
                __syncthreads();
                if (tid < qn - kSphThreads) s_queue[tid] = s_queue[kSphThreads + tid];
                qn -= kSphThreads;
                __syncthreads();
            }
        }
        __syncthreads();                               // s_pref / s_row are rewritten by the next rows
    }
    if (qn > 0) process(tid < qn ? s_queue[tid] : -1);

    // fixed-order block sums: a butterfly inside each wave, then the waves in order
#pragma unroll
    for (int j = 0; j < kSlots; ++j)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double c = wave_sum(accC[j][g]), sv = wave_sum(accS[j][g]);
            if (lane == 0) { s_red[wave][(j * G + g) * 2] = c; s_red[wave][(j * G + g) * 2 + 1] = sv; }
        }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const double ev = wave_sum(accE[g]);
        if (lane == 0) s_red[wave][2 * kSlots * G + g] = ev;
    }
    int cnt = count;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    const int C = (lmax + 1) * (lmax + 1);
    for (int v = tid; v < kNv; v += kSphThreads) {
        double sum = s_red[0][v];
        for (int w = 1; w < kSphWaves; ++w) sum += s_red[w][v];
        if (v < 2 * kSlots * G) {
            const int j = v / (2 * G), g = (v / 2) % G, part = v & 1;
            if (j >= nslots || g0 + g >= a.ngrids) continue;
            const int m = j < na ? ma : mb, l = j < na ? ma + j : mb + j - na;
            if (part == 1 && m == 0) continue;
            const int c = l * l + l + (part ? -m : m);
            a.coeffs[((long)(g0 + g) * a.nshell + s) * C + c] = sum;
        } else {
            const int g = v - 2 * kSlots * G;
            if (group == 0 && g0 + g < a.ngrids) a.shell_energy[(long)(g0 + g) * a.nshell + s] = sum;
        }
    }
    if (tid == 0 && group == 0 && blockIdx.z == 0) {
        long long n = 0;
        for (int w = 0; w < kSphWaves; ++w) n += s_cnt[w];
        a.shell_nodes[s] = n;
    }
}

template <int LMAX_T, int G, int NT>
hipError_t launch_sph(const SphArgs &a, hipStream_t stream)
{
    const dim3 grid((unsigned)(1 + (a.lmax + 1) / 2), (unsigned)a.nshell, (unsigned)((a.ngrids + G - 1) / G));
    hipLaunchKernelGGL((k_sph_modes<LMAX_T, G, NT>), grid, dim3(NT), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sph_modes(const SphArgs &a, hipStream_t stream)
{
    // with several grids, four share a block's harmonic work (their accumulators take ~360 registers: one wave per SIMD);
    // at lmax > 16 one grid's accumulators are enough.  One grid per block leaves room for 8 waves per block (<= 256
    // registers): a block is a serial chain over its shell's rows, and twice the waves take it in half the steps.
    if (a.lmax <= 16) return a.ngrids > 1 ? launch_sph<16, 4, 256>(a, stream) : launch_sph<16, 1, 512>(a, stream);
    return launch_sph<32, 1, 512>(a, stream);
}

}  // namespace cbet
