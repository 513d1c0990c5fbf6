"""Anderson mixing of the gain iterate off the GPU: the coefficient solve, the host twins of the two
streaming passes against a numpy restatement, cbet_fixed_point with the host mixing on a linear toy map (where Anderson mixing
with full memory is GMRES), the restart rule, the oracle engine's solve on one rank and on two over gloo, and the twins under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program.

Bounds: bit for bit where both sides run the same IEEE statements (f, the combination); 1e-12 of sum |a b| for a dot product
summed in two orders (the twins' blocked order against math.fsum)."""
import json
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, load_inputs
from helpers import mixing_cases as MC
from helpers.twin_driver import run_driver


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


# ---- 1. coefficients ---------------------------------------------------------------------------------------------------
def _gram(fs):
    return np.array([[float(np.dot(a, b)) for b in fs] for a in fs])


def test_coefficients(api):
    alpha, dropped = api.mix_coefficients(np.array([[3.7]]))
    assert alpha.tolist() == [1.0] and dropped == 0
    rng = np.random.default_rng(11)
    f_old, f_new = rng.standard_normal(50), rng.standard_normal(50)
    G = _gram([f_old, f_new])
    alpha, dropped = api.mix_coefficients(G)
    # minimise |a f_old + (1 - a) f_new|^2: a = <f_new - f_old, f_new> / |f_old - f_new|^2
    want = (G[1, 1] - G[0, 1]) / (G[0, 0] - 2.0 * G[0, 1] + G[1, 1])
    assert dropped == 0 and abs(alpha[0] - want) <= 4e-16 * abs(want) and abs(alpha.sum() - 1.0) <= 4e-16
    for count in (3, 4, 5):
        fs = [rng.standard_normal(40) for _ in range(count)]
        alpha, dropped = api.mix_coefficients(_gram(fs))
        assert dropped == 0 and np.isfinite(alpha).all() and abs(alpha.sum() - 1.0) <= 1e-14 * np.abs(alpha).sum()
        mixed = sum(a * f for a, f in zip(alpha, fs))
        for k in range(count - 1):      # the minimiser: its residual is orthogonal to every difference against the newest
            diff = fs[k] - fs[-1]
            assert abs(np.dot(mixed, diff)) <= 1e-12 * np.linalg.norm(mixed) * np.linalg.norm(diff) + 1e-13 * np.abs(mixed * diff).sum()
        a2, d2 = api.mix_coefficients(_gram(fs))
        assert MC.same_bytes(a2, alpha) and d2 == dropped            # pure host arithmetic: the same bytes again
    # the oldest residual twice: the Gram matrix cannot tell entries 0 and 1 apart; exactly the oldest goes
    fs = [rng.standard_normal(40) for _ in range(3)]
    fs = [fs[0].copy()] + fs
    alpha, dropped = api.mix_coefficients(_gram(fs))
    assert dropped == 1 and alpha[0] == 0.0 and np.isfinite(alpha).all() and abs(alpha.sum() - 1.0) <= 1e-14 * np.abs(alpha).sum()
    kept, _ = api.mix_coefficients(_gram(fs[1:]))
    assert MC.same_bytes(alpha[1:], kept)
    for bad in (np.zeros((0, 0)), np.zeros((6, 6))):
        with pytest.raises(api.CbetError) as ei:
            api.mix_coefficients(bad)
        assert ei.value.code == api.EINVAL


# ---- 2. the twins against numpy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", MC.SIZES)
def test_twins_match_numpy(api, n):
    for h in range(api.MIX_MAX_DEPTH + 1):
        y, x, *held = MC.arrays(n, h, seed=100 * n + h)
        want_f, want_row, scale = MC.residual_numpy(y, x, held)
        f = np.full(n, np.nan)
        row = api.mix_residual_host(y, x, f, held)
        assert MC.same_bytes(f, want_f), (n, h)
        err = np.abs(row - want_row)
        print("n %d h %d: row error / sum|ab| = %s" % (n, h, (err / scale).tolist()))
        assert (err <= 1e-12 * scale).all(), (n, h, err / scale)
        assert MC.same_bytes(api.mix_residual_host(y, x, np.empty(n), held), row)
        # the combination of h + 1 entries, oldest first
        entries = held + [y]
        alpha = np.random.default_rng(n + h).standard_normal(h + 1)
        alpha[-1] = 1.0 - alpha[:-1].sum()
        want = MC.apply_numpy(entries, alpha)
        out, keep = np.full(n, np.nan), np.full(n, np.nan)
        api.mix_apply_host(entries, alpha, out, keep)
        assert MC.same_bytes(out, want) and MC.same_bytes(keep, want), (n, h)
        alias = [e.copy() for e in entries]
        api.mix_apply_host(alias, alpha, alias[0])                  # x_out is the oldest slot, no x_keep
        assert MC.same_bytes(alias[0], want) and all(MC.same_bytes(a, e) for a, e in zip(alias[1:], entries[1:]))
    out = np.full(n, np.nan)
    api.mix_apply_host([y], [1.0], out)
    assert MC.same_bytes(out, y)                                    # alpha = {1.0}: y's bytes


def test_twin_argument_errors(api):
    a = np.zeros(4)
    for call in (lambda: api.mix_residual_host(a, a, np.zeros(4), [a] * 5),
                 lambda: api.mix_residual_host(a, a, np.zeros(4), [], n=-1),
                 lambda: api.mix_residual_host(a, None, np.zeros(4), []),
                 lambda: api.mix_apply_host([], [], np.zeros(4)),
                 lambda: api.mix_apply_host([a] * 6, [0.0] * 6, np.zeros(4)),
                 lambda: api.mix_apply_host([a], [1.0], np.zeros(4), n=-1),
                 lambda: api.mix_apply_host([a], [1.0], None, n=4)):
        with pytest.raises(api.CbetError) as ei:
            call()
        assert ei.value.code == api.EINVAL and "cbet_mix" in str(ei.value)
    assert api.mix_work_bytes(-1) == 0 and api.mix_work_bytes(1) == 8 * (api.MIX_MAX_DEPTH + 1)
    assert api.mix_work_bytes(api.MIX_SPAN * api.MIX_MAX_GROUPS * 3) == 8 * (api.MIX_MAX_DEPTH + 1) * api.MIX_MAX_GROUPS


# ---- 3. a linear toy map: Anderson mixing with full memory is GMRES ------------------------------------------------------
def _toy(relax, values, seed, **kw):
    rng = np.random.default_rng(seed)
    d = rng.choice(np.array(values), 1000)
    return MC.ToyEngine(d, rng.standard_normal(1000), relax, **kw)


@pytest.mark.parametrize("relax,values", [(0.5, (0.9, -0.5, 0.3)), (1.0, (0.9, -0.5, 0.3)), (0.5, (0.8, 0.1, -0.7))])
def test_toy_map_is_solved_in_four_mixed_passes(api, relax, values):
    from cbet_raytracing_3d_amd.cbet_loop import cbet_fixed_point
    gp = api.default_gain_params(relax=relax, tolerance=1e-300, max_passes=8)
    eng = _toy(relax, values, seed=5)
    rep = cbet_fixed_point(eng, gp, mixing=3)
    mix = rep["mixing"]
    res = mix["residual_l2"]
    print("relax %g, eigenvalues %s: residual_l2 %s, held %s" % (relax, values, res, mix["held"]))
    assert rep["passes"] >= 6 and len(res) == rep["passes"] - gp.direction_passes == len(mix["held"])
    assert mix["depth"] == 3 and max(mix["held"]) <= 4 and mix["held"][:4] == [1, 2, 3, 4]
    assert mix["bytes"] == 8 * 1000 * 9
    assert res[0] == pytest.approx(eng.res[gp.direction_passes], rel=1e-14)
    # three distinct eigenvalues: the fourth mixed iterate is the fixed point
    assert res[4] <= 1e-9 * res[0], res
    plain = _toy(relax, values, seed=5)
    rep0 = cbet_fixed_point(plain, gp, mixing=0)
    assert "mixing" not in rep0
    if relax == 0.5 and 0.9 in values:
        # the lambda = 0.9 component shrinks by 0.95 per pass: without mixing the fifth residual is most of the first
        assert plain.res[gp.direction_passes + 4] >= 0.38 * plain.res[gp.direction_passes]
    assert np.abs(eng.gain - (eng.b / (1.0 - eng.d))).max() <= 1e-9 * np.abs(eng.gain).max()


# ---- 4. restart -----------------------------------------------------------------------------------------------------------
def test_a_grown_residual_restarts_with_the_plain_step(api):
    from cbet_raytracing_3d_amd.cbet_loop import cbet_fixed_point
    gp = api.default_gain_params(relax=0.5, tolerance=1e-300, max_passes=8)
    rng = np.random.default_rng(9)
    eng = _toy(0.5, (0.9, -0.5, 0.3), seed=5, switch_at=4, b2=30.0 * rng.standard_normal(1000))   # another map from update 4 on
    rep = cbet_fixed_point(eng, gp, mixing=3)
    mix = rep["mixing"]
    print("held %s restarts %d residual_l2 %s" % (mix["held"], mix["restarts"], mix["residual_l2"]))
    k = 4 - gp.direction_passes                # the frozen pass whose update ran the new map first
    assert mix["restarts"] == 1 and mix["held"][:k + 2] == [1, 2, 3, 1, 2]
    assert mix["residual_l2"][k] > mix["residual_l2"][k - 1]
    assert mix["alpha_history"][k] == [1.0]
    # the step after the restart is the plain step: update 5 started from the bytes update 4 made
    assert MC.same_bytes(eng.seen[5], eng.made[4])
    assert not MC.same_bytes(eng.seen[4], eng.made[3])          # (the step before it was a mixed one)


# ---- 5. the oracle engine's solve with the host mixing ----------------------------------------------------------------------
def _oracle_solve(rank, world, group=None):
    sys.path.insert(0, ROOT)
    from cbet_raytracing_3d_amd import api
    from cbet_raytracing_3d_amd.cbet_loop import cbet_fixed_point
    from oracle import cbet_oracle as O
    from test_cbet_model import BEAMS, N
    bn, r, ne, te = load_inputs()
    cfg = O.default_config(N, nbeams=len(BEAMS))
    ne3d, kap = O.node_tables(cfg, r, ne, te)
    eng = MC.mixed_oracle_engine(O, api, cfg, O.gain_default(), bn[BEAMS].copy(), ne3d, kap, len(BEAMS))
    gp = api.default_gain_params(relax=1.0, tolerance=1e-5, max_passes=8)      # test_cbet_model._solve's
    return cbet_fixed_point(eng, gp, rank, world, group, mixing=2), gp


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rep, _ = _oracle_solve(rank, world)
        with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as fh:
            json.dump({"passes": rep["passes"], "converged": bool(rep["converged"]), "imbalance": rep["imbalance"],
                       "alpha": [[a.hex() for a in step] for step in rep["mixing"]["alpha_history"]],
                       "held": rep["mixing"]["held"], "restarts": rep["mixing"]["restarts"]}, fh)
    finally:
        dist.destroy_process_group()


def test_oracle_engine_solve_with_mixing(api, oracle):
    rep, gp = _oracle_solve(0, 1)
    mix = rep["mixing"]
    print("passes %d change %.3g imbalance %.3g held %s restarts %d dropped %d residual_l2 %s" % (
        rep["passes"], rep["change"], rep["imbalance"], mix["held"], mix["restarts"], mix["dropped"], mix["residual_l2"]))
    assert rep["converged"] and rep["passes"] <= gp.max_passes
    assert rep["imbalance"] < 1e-3                                   # test_sharded_iteration_equals_unsharded's bound
    assert max(mix["held"]) <= 3 and len(mix["residual_l2"]) == rep["passes"] - gp.direction_passes


def test_two_ranks_take_the_same_mixed_steps(tmp_path, api, oracle):
    port = 29950 + (os.getpid() % 40)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (json.load(open(tmp_path / ("rank%d.json" % r))) for r in (0, 1))
    assert r0["converged"] and r1["converged"] and r0["passes"] == r1["passes"]
    assert r0["alpha"] == r1["alpha"] and len(r0["alpha"]) >= 1     # hex strings: bit for bit
    assert r0["held"] == r1["held"] and r0["restarts"] == r1["restarts"]
    assert r0["imbalance"] < 1e-3 and r1["imbalance"] < 1e-3


# ---- 6. the twins under the sanitizers -----------------------------------------------------------------------------------
DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "cbet_mi355x.h"

#define REQUIRE(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s: ", #cond); std::fprintf(stderr, __VA_ARGS__); \
                                               std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

static double *block(size_t n) { double *p = (double *)std::malloc(n * sizeof(double)); REQUIRE(p, "malloc"); return p; }
static bool same(const double *a, const double *b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }
static double value(long e, int k) { return std::sin(0.37 * e + 1.3 * k) * (1.0 + (e % 7)) + 0.01 * k; }

int main()
{
    const long sizes[] = {1, 63, 64, 65, 255, 2 * CBET_MIX_SPAN + 3};       // every array a heap block of exactly n doubles
    double checksum = 0.0;
    for (long n : sizes)
        for (int h = 0; h <= CBET_MIX_MAX_DEPTH; ++h) {
            double *y = block(n), *x = block(n), *f = block(n), *out = block(n), *keep = block(n), *row = block(h + 1);
            double *held[CBET_MIX_MAX_DEPTH + 1];
            for (int j = 0; j < h; ++j) held[j] = block(n);
            for (long e = 0; e < n; ++e) {
                y[e] = value(e, 0); x[e] = value(e, 1);
                for (int j = 0; j < h; ++j) held[j][e] = value(e, 2 + j);
            }
            REQUIRE(cbet_mix_residual_host(y, x, f, h ? held : nullptr, h, n, row) == CBET_OK, "%s", cbet_last_error());
            double naive[CBET_MIX_MAX_DEPTH + 1] = {}, scale[CBET_MIX_MAX_DEPTH + 1] = {};
            for (long e = 0; e < n; ++e) {
                const double d = y[e] - x[e];
                REQUIRE(same(&f[e], &d, 1), "n %ld h %d: f[%ld]", n, h, e);
                for (int j = 0; j <= h; ++j) { const double t = d * (j < h ? held[j][e] : d); naive[j] += t; scale[j] += std::fabs(t); }
            }
            for (int j = 0; j <= h; ++j) {
                REQUIRE(std::fabs(row[j] - naive[j]) <= 1e-12 * scale[j], "n %ld h %d: row[%d] %a vs %a", n, h, j, row[j], naive[j]);
                checksum += row[j];
            }
            // the combination of h + 1 entries: into fresh blocks, then into the oldest slot
            double alpha[CBET_MIX_MAX_DEPTH + 1], sum = 0.0;
            for (int j = 0; j < h; ++j) { alpha[j] = 0.3 - 0.2 * j; sum += alpha[j]; }
            alpha[h] = 1.0 - sum;
            held[h] = y;
            REQUIRE(cbet_mix_apply_host(held, alpha, h + 1, n, out, keep) == CBET_OK, "%s", cbet_last_error());
            REQUIRE(same(out, keep, n), "n %ld h %d: x_keep", n, h);
            REQUIRE(cbet_mix_apply_host(held, alpha, h + 1, n, held[0], nullptr) == CBET_OK, "%s", cbet_last_error());
            REQUIRE(same(held[0], out, n), "n %ld h %d: x_out = the oldest slot", n, h);
            checksum += out[n - 1];
            for (int j = 0; j < h; ++j) std::free(held[j]);
            std::free(y); std::free(x); std::free(f); std::free(out); std::free(keep); std::free(row);
        }
    // coefficients: one entry, five entries, the oldest twice
    for (int count = 1; count <= CBET_MIX_MAX_DEPTH + 1; ++count) {
        double *gram = block((size_t)count * count), *alpha = block(count);
        for (int a = 0; a < count; ++a)
            for (int b = 0; b < count; ++b) {
                double s = 0.0;
                const int ka = (count >= 3 && a == 0) ? 1 : a, kb = (count >= 3 && b == 0) ? 1 : b;   // three and more: entry 0 = entry 1
                for (long e = 0; e < 97; ++e) s += value(e, ka) * value(e, kb);
                gram[a * count + b] = s;
            }
        int dropped = -1;
        REQUIRE(cbet_mix_coefficients(gram, count, alpha, &dropped) == CBET_OK, "%s", cbet_last_error());
        REQUIRE(dropped == (count >= 3 ? 1 : 0), "count %d: dropped %d", count, dropped);
        double sum = 0.0;
        for (int a = 0; a < count; ++a) { REQUIRE(std::isfinite(alpha[a]), "alpha[%d]", a); sum += alpha[a]; }
        REQUIRE(std::fabs(sum - 1.0) < 1e-9, "count %d: sum alpha %g", count, sum);
        std::free(gram); std::free(alpha);
    }
    double one = 1.0, *p = &one;
    int dropped = 0;
    REQUIRE(cbet_mix_residual_host(p, p, p, nullptr, 5, 1, p) == CBET_EINVAL, "h = 5");
    REQUIRE(cbet_mix_residual_host(p, p, p, nullptr, 0, -1, p) == CBET_EINVAL, "n < 0");
    REQUIRE(cbet_mix_residual_host(p, nullptr, p, nullptr, 0, 1, p) == CBET_EINVAL, "NULL x");
    REQUIRE(cbet_mix_apply_host(&p, p, 0, 1, p, nullptr) == CBET_EINVAL, "count 0");
    REQUIRE(cbet_mix_coefficients(p, 0, p, &dropped) == CBET_EINVAL && std::strstr(cbet_last_error(), "count"), "count 0");
    std::printf("mix twins ok: checksum %.17g\n", checksum);
    return 0;
}
'''


def test_twins_stay_in_bounds_under_asan_ubsan(tmp_path):
    out = run_driver(tmp_path, DRIVER, sources=("cbet_mix_host.cpp", "cbet_params.cpp"))
    assert "mix twins ok" in out
