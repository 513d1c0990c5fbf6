// cbet_mix_host.cpp -- the host side of the Anderson mixing of the gain iterate (include/cbet_mi355x.h):
// the twins of k_mix_residual / k_mix_reduce and k_mix_apply, which run cbet_mix_model.h's statements in the kernels' own order
// (a Gram row has the device's bytes), the coefficient solve, and the refusals the device entries (cbet_mix.hip) share.  No HIP
// call: this file links without the runtime, and the twins are the reference of the device path at any size.
#include <cmath>
#include <cstring>
#include <vector>

#include "cbet_host_internal.h"
#include "cbet_mix_model.h"

namespace cbet {

int mix_residual_check(const char *who, const double *y, const double *x, const double *f, const double *const *f_held, int h,
                       long n, const double *row)
{
    if (h < 0 || h > CBET_MIX_MAX_DEPTH) return fail(CBET_EINVAL, "%s: h = %d held residuals outside 0 .. %d", who, h, CBET_MIX_MAX_DEPTH);
    if (n < 0) return fail(CBET_EINVAL, "%s: n = %ld is negative", who, n);
    if (!y || !x || !f) return fail(CBET_EINVAL, "%s: %s is NULL", who, !y ? "y" : (!x ? "x" : "f"));
    if (!row) return fail(CBET_EINVAL, "%s: row is NULL", who);
    if (h > 0 && !f_held) return fail(CBET_EINVAL, "%s: f_held is NULL with h = %d", who, h);
    for (int j = 0; j < h; ++j)
        if (!f_held[j]) return fail(CBET_EINVAL, "%s: f_held[%d] is NULL", who, j);
    return CBET_OK;
}

int mix_apply_check(const char *who, const double *const *y_held, const double *alpha, int count, long n, const double *x_out)
{
    if (count < 1 || count > CBET_MIX_MAX_DEPTH + 1)
        return fail(CBET_EINVAL, "%s: count = %d entries outside 1 .. %d", who, count, CBET_MIX_MAX_DEPTH + 1);
    if (n < 0) return fail(CBET_EINVAL, "%s: n = %ld is negative", who, n);
    if (!y_held || !alpha || !x_out) return fail(CBET_EINVAL, "%s: %s is NULL", who, !y_held ? "y_held" : (!alpha ? "alpha" : "x_out"));
    for (int j = 0; j < count; ++j)
        if (!y_held[j]) return fail(CBET_EINVAL, "%s: y_held[%d] is NULL", who, j);
    return CBET_OK;
}

namespace {

// 256 thread sums -> one, as a workgroup of the kernels does it: six butterfly steps per wavefront (every lane ends with the
// wavefront's sum: the adds commute), then the wavefronts in order.
double workgroup_sum(const double *v)
{
    double part[kMixThreads / kMixWave];
    for (int w = 0; w < kMixThreads / kMixWave; ++w) {
        double a[kMixWave], b[kMixWave];
        std::memcpy(a, v + w * kMixWave, sizeof a);
        for (int off = kMixWave / 2; off > 0; off >>= 1) {
            for (int l = 0; l < kMixWave; ++l) b[l] = a[l] + a[l ^ off];
            std::memcpy(a, b, sizeof a);
        }
        part[w] = a[0];
    }
    double t = part[0];
    for (int w = 1; w < kMixThreads / kMixWave; ++w) t = t + part[w];
    return t;
}

template <int H>
void residual_host(const double *y, const double *x, double *f, const double *const *f_held, long n, double *row)
{
    const long spans = mix_spans(n), groups = mix_groups(n);
    std::vector<double> work((size_t)groups * kMixRow, 0.0);
    std::vector<double> acc((size_t)kMixThreads * (H + 1)), column(kMixThreads);
    for (long g = 0; g < groups; ++g) {                       // k_mix_residual, workgroup g
        std::fill(acc.begin(), acc.end(), 0.0);
        for (long s = g; s < spans; s += groups)
            for (int i = 0; i < kMixIters; ++i)
                for (int t = 0; t < kMixThreads; ++t)
                    for (long e = mix_element(s, i, t), last = e + 1; e <= last && e < n; ++e) {
                        double fh[H > 0 ? H : 1];
                        for (int j = 0; j < H; ++j) fh[j] = f_held[j][e];
                        f[e] = mix_residual_element<H>(y[e], x[e], fh, &acc[(size_t)t * (H + 1)]);
                    }
        for (int j = 0; j <= H; ++j) {
            for (int t = 0; t < kMixThreads; ++t) column[t] = acc[(size_t)t * (H + 1) + j];
            work[(size_t)g * kMixRow + j] = workgroup_sum(column.data());
        }
    }
    for (int j = 0; j <= H; ++j) {                            // k_mix_reduce
        for (int t = 0; t < kMixThreads; ++t) {
            double s = 0.0;
            for (long g = t; g < groups; g += kMixThreads) s = s + work[(size_t)g * kMixRow + j];
            column[t] = s;
        }
        row[j] = workgroup_sum(column.data());
    }
}

template <int C>
void apply_host(const double *const *y_held, const double *alpha, long n, double *x_out, double *x_keep)
{
    for (long e = 0; e < n; ++e) {
        double y[C];
        for (int j = 0; j < C; ++j) y[j] = y_held[j][e];      // every entry read before x_out (maybe one of them) is written
        const double v = mix_combine<C>(y, alpha);
        x_out[e] = v;
        if (x_keep) x_keep[e] = v;
    }
}

}  // namespace
}  // namespace cbet

extern "C" size_t cbet_mix_work_bytes(long n)
{
    return n < 0 ? 0 : (size_t)cbet::mix_groups(n) * cbet::kMixRow * sizeof(double);
}

extern "C" int cbet_mix_residual_host(const double *y, const double *x, double *f, const double *const *f_held, int h, long n,
                                      double *row)
{
    using namespace cbet;
    if (int rc = mix_residual_check("cbet_mix_residual_host", y, x, f, f_held, h, n, row)) return rc;
    switch (h) {
    case 0: residual_host<0>(y, x, f, f_held, n, row); break;
    case 1: residual_host<1>(y, x, f, f_held, n, row); break;
    case 2: residual_host<2>(y, x, f, f_held, n, row); break;
    case 3: residual_host<3>(y, x, f, f_held, n, row); break;
    default: residual_host<4>(y, x, f, f_held, n, row); break;
    }
    return CBET_OK;
}

extern "C" int cbet_mix_apply_host(const double *const *y_held, const double *alpha, int count, long n, double *x_out, double *x_keep)
{
    using namespace cbet;
    if (int rc = mix_apply_check("cbet_mix_apply_host", y_held, alpha, count, n, x_out)) return rc;
    switch (count) {
    case 1: apply_host<1>(y_held, alpha, n, x_out, x_keep); break;
    case 2: apply_host<2>(y_held, alpha, n, x_out, x_keep); break;
    case 3: apply_host<3>(y_held, alpha, n, x_out, x_keep); break;
    case 4: apply_host<4>(y_held, alpha, n, x_out, x_keep); break;
    default: apply_host<5>(y_held, alpha, n, x_out, x_keep); break;
    }
    return CBET_OK;
}

extern "C" int cbet_mix_coefficients(const double *gram, int count, double *alpha, int *dropped)
{
    using namespace cbet;
    if (count < 1 || count > CBET_MIX_MAX_DEPTH + 1)
        return fail(CBET_EINVAL, "cbet_mix_coefficients: count = %d entries outside 1 .. %d", count, CBET_MIX_MAX_DEPTH + 1);
    if (!gram || !alpha || !dropped)
        return fail(CBET_EINVAL, "cbet_mix_coefficients: %s is NULL", !gram ? "gram" : (!alpha ? "alpha" : "dropped"));
    const int n = count - 1;
    auto G = [&](int a, int b) { return a <= b ? gram[a * count + b] : gram[b * count + a]; };
    const double Gnn = G(n, n);
    int d = 0;
    for (;; ++d) {
        // the differences in use, newest first: row r is entry n - 1 - r, m = n - d of them
        const int m = n - d;
        double L[CBET_MIX_MAX_DEPTH][CBET_MIX_MAX_DEPTH], c[CBET_MIX_MAX_DEPTH], gamma[CBET_MIX_MAX_DEPTH];
        bool lost = false;
        for (int r = 0; r < m && !lost; ++r) {
            const int a = n - 1 - r;
            c[r] = Gnn - G(a, n);
            for (int q = 0; q <= r; ++q) {
                const int b = n - 1 - q;
                double v = ((G(a, b) - G(a, n)) - G(b, n)) + Gnn;      // H_ab
                const double diag = v;
                for (int k = 0; k < q; ++k) v = v - L[r][k] * L[q][k];
                if (q < r) {
                    L[r][q] = v / L[q][q];
                } else if (!(v > 1e-12 * diag)) {
                    lost = true;                                       // (a NaN pivot or diagonal is lost too)
                } else {
                    L[r][r] = std::sqrt(v);
                }
            }
        }
        if (lost) continue;                                            // drop the oldest entry and solve again (m = 0 never loses)
        for (int r = 0; r < m; ++r) {                                  // L z = c
            double v = c[r];
            for (int k = 0; k < r; ++k) v = v - L[r][k] * gamma[k];
            gamma[r] = v / L[r][r];
        }
        for (int r = m - 1; r >= 0; --r) {                             // L^T gamma = z
            double v = gamma[r];
            for (int k = r + 1; k < m; ++k) v = v - L[k][r] * gamma[k];
            gamma[r] = v / L[r][r];
        }
        double sum = 0.0;
        for (int r = 0; r < m; ++r) sum = sum + gamma[r];
        for (int a = 0; a < d; ++a) alpha[a] = 0.0;
        for (int r = 0; r < m; ++r) alpha[n - 1 - r] = gamma[r];
        alpha[n] = 1.0 - sum;
        *dropped = d;
        return CBET_OK;
    }
}
