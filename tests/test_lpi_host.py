"""The quarter-critical LPI maps, the part that needs no device: the new entries of the C ABI are exported,
declared and refuse bad arguments, and the host twin cbet_lpi_map_host -- the reference of the device path in
tests/test_gpu_lpi.py -- agrees with a numpy restatement written from the header's text (helpers/lpi_cases.py) on its three
cases (TRACED, CROWDED with two bands, RAMP) and keeps the model's exact properties.

Bounds: LAST_BITS = 1e-12 relative, per cell and quantity, between the twin and the restatement (two formulations of one
quantity); counts and argmax_cw exact.  A cell may be left out of the I_cw / eta_cw comparison where a present beam's
(1 - mu) NB / 2 lies within 1e-9 of an integer -- at most 1 % of a case's band cells, none on TRACED.  What the model makes
exact is asserted bitwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import NCPU, ROOT
from helpers import lpi_cases as LC
from helpers.gain_worlds import LAST_BITS
from helpers.lpi_cases import BAND, ETA_CW, ETA_SUM, I_CW, I_MAX, I_SUM, LN

NAMES = ("cbet_lpi_work_bytes", "cbet_lpi_summary_init", "cbet_lpi_map", "cbet_lpi_map_host")


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module")
def cases(api, oracle, inputs):
    return {"traced": LC.traced_case(api, oracle, inputs, NCPU), "crowded": LC.crowded_case(api, oracle, inputs, NCPU),
            "crowded_wide": LC.crowded_case(api, oracle, inputs, NCPU, wide=True), "ramp": LC.ramp_case(api)}


def _error(api):
    return api.lib().cbet_last_error().decode()


def _twin(api, c, fields=None, **kw):
    args = dict(te=c["te"], band=c["band"], cone_bins=c["nbins"])
    args.update(kw)
    return api.lpi_map_host(c["fields"] if fields is None else fields, c["ne3d"], c["p"], **args)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound(api):
    header = open(os.path.join(ROOT, "include", "cbet_mi355x.h")).read()
    for name in NAMES:
        assert ("%s(" % name) in header
    assert callable(api.lpi_map) and callable(api.lpi_map_host) and callable(api.lpi_work_bytes)
    from cbet_raytracing_3d_amd import lpi
    from cbet_raytracing_3d_amd.tracer import RayTracer
    assert callable(RayTracer.lpi_map) and callable(lpi.srs_parameter) and callable(lpi.surface_means) and callable(lpi.summarize)
    assert "quarter-critical LPI maps" in header and "UNPINNED" in header.split("quarter-critical LPI maps")[1].split("exit pass")[0]
    assert (api.LPI_BAND, api.LPI_I_SUM, api.LPI_I_CW, api.LPI_I_MAX, api.LPI_LN, api.LPI_ETA_SUM, api.LPI_ETA_CW) == tuple(range(7))
    for q, name in enumerate(("BAND", "I_SUM", "I_CW", "I_MAX", "LN", "ETA_SUM", "ETA_CW")):
        assert "#define CBET_LPI_%s %d\n" % (name, q) in header
    assert C.sizeof(api.LpiSummary) == api.LPI_SUMMARY_BYTES == 96
    model = open(os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc", "cbet_lpi_model.h")).read()
    assert "UNPINNED" in model


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "cbet_mi355x.h"\n'
                   "int dev(const double *f, double *o, cbet_lpi_summary *s, void *w, const cbet_params *p, cbet_context *c)\n"
                   "{ return cbet_lpi_work_bytes(p) ? cbet_lpi_map(f, 0, 0, 1000.0, 0.2, 0.25, 8, o, s, w, 0, 2, p, c, 0) : 0; }\n"
                   "int host(const double *f, const double *n, double *o, const cbet_params *p)\n"
                   "{ cbet_lpi_summary s; cbet_lpi_summary_init(&s); return cbet_lpi_map_host(f, n, 0, 1000.0, 0.2, 0.25, 8, o, &s, 0, 2, p); }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_work_bytes_follow_the_slab_alone(api):
    from helpers import gain_worlds as W
    for shape, nb in (((6, 9, 13), 2), ((13, 11, 148), 60), ((48, 21, 134), 6), ((256, 256, 256), 60)):
        p = W.params(api, shape, nb)
        bricks = ((shape[0] + 3) >> 1) * ((shape[1] + 5) // 4) * ((shape[2] + 9) // 8)
        assert api.lpi_work_bytes(p) == min((bricks + 3) // 4, 8192) * 96, (shape, nb)
    assert api.lpi_work_bytes(W.params(api, (5, 4, 37), 65)) == 0
    assert api.lib().cbet_lpi_work_bytes(None) == 0


def test_summary_init(api):
    s = api.lpi_summary_new().as_dict()
    assert s.pop("argmax_cw") == -1 and all(v == 0 for v in s.values())
    assert api.lib().cbet_lpi_summary_init(None) == api.EINVAL and "summary is NULL" in _error(api)


def test_both_entries_refuse_bad_arguments_and_name_them(api):
    """The arguments are judged before the context: the refusals do not need a device."""
    p = api.default_params(16)
    L = api.lib()

    def dev(f=8, te3d=None, te=1000.0, lo=0.2, hi=0.25, nb=8, o=8, s=None, w=None, x0=0, x1=18, pp=p):
        return L.cbet_lpi_map(f, None, te3d, te, lo, hi, nb, o, s, w, x0, x1, C.byref(pp), None, None)

    def host(f=8, ne=8, te3d=None, te=1000.0, lo=0.2, hi=0.25, nb=8, o=8, x0=0, x1=18, pp=p):
        return L.cbet_lpi_map_host(f, ne, te3d, te, lo, hi, nb, o, None, x0, x1, C.byref(pp))

    for call, who in ((dev, "cbet_lpi_map:"), (host, "cbet_lpi_map_host:")):
        assert call(f=None) == api.EINVAL and "fields is NULL" in _error(api) and who in _error(api)
        assert call(o=None) == api.EINVAL and "lpi is NULL" in _error(api)
        for lo, hi in ((-0.1, 0.25), (0.3, 0.25), (0.2, 1.0), (float("nan"), 0.25), (0.2, float("nan"))):
            assert call(lo=lo, hi=hi) == api.EINVAL and "band" in _error(api) and "frac_lo" in _error(api), (lo, hi)
        for nb in (0, 17, -3):
            assert call(nb=nb) == api.EINVAL and "cone_bins = %d" % nb in _error(api)
        assert call(pp=api.default_params(16, nbeams=65)) == api.EINVAL
        assert "nbeams = 65" in _error(api) and "CBET_MAX_CBET_BEAMS" in _error(api)
        for te in (0.0, -5.0, float("nan")):
            assert call(te=te) == api.EINVAL and "te_ev" in _error(api)
        for x0, x1 in ((-1, 4), (0, 19), (5, 4)):
            assert call(x0=x0, x1=x1) == api.EINVAL and "slab [%d,%d)" % (x0, x1) in _error(api)
    assert host(ne=None) == api.EINVAL and "ne3d is NULL" in _error(api)
    assert dev(s=8) == api.EINVAL and "work is NULL" in _error(api)
    assert dev() == api.EINVAL and "NULL context" in _error(api)                      # every argument fine but the context
    assert dev(te=0.0, te3d=8) == api.EINVAL and "NULL context" in _error(api)        # a table makes te_ev irrelevant
    assert L.cbet_lpi_map(8, None, None, 1000.0, 0.2, 0.25, 8, 8, None, None, 0, 18, None, None, None) == api.EINVAL


# ---- the twin against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["traced", "crowded", "crowded_wide", "ramp"])
def test_twin_matches_the_restatement(api, cases, name):
    c = cases[name]
    got, s = _twin(api, c)
    ref, rs, near = c["ref"], c["ref_summary"], c["near"]
    band = ref[BAND] > 0
    assert np.array_equal(got[BAND], ref[BAND])
    assert not got[:, ~band].any()                                                      # out of band: exactly 0 everywhere
    left_out = int(near.sum())
    print("%s: %d band cells, %d left out of the I_cw comparison" % (name, rs["band_cells"], left_out))
    assert left_out <= 0.01 * rs["band_cells"] and (name != "traced" or left_out == 0)
    for q in (I_SUM, I_CW, I_MAX, LN, ETA_SUM, ETA_CW):
        keep = band & ~near if q in (I_CW, ETA_CW) else band
        err = np.abs(got[q][keep] - ref[q][keep])
        worst = float((err / np.where(ref[q][keep] != 0, np.abs(ref[q][keep]), 1.0)).max())
        print("  quantity %d: worst relative difference %.3e" % (q, worst))
        assert (err <= LAST_BITS * np.abs(ref[q][keep])).all(), (name, q, worst)
    for k in LC.COUNTS:
        if k == "argmax_cw" and left_out:
            continue
        assert s[k] == rs[k], (k, s[k], rs[k])
    for k in LC.MAXIMA + LC.SUMS:
        if left_out and k in ("max_eta_cw", "sum_I_cw"):
            continue
        assert abs(s[k] - rs[k]) <= LAST_BITS * abs(rs[k]), (k, s[k], rs[k])


def test_ramp_is_analytic_and_its_bins_are_exact(api, cases):
    c = cases["ramp"]
    got, s = _twin(api, c)
    band = got[BAND] > 0
    want = c["dz"] / np.sinh(c["dz"] / c["L"])                                      # (ne[k+1] - ne[k-1]) / (2 dz) of an exponential
    ln = got[LN][band]
    assert float(np.abs(ln - want).max()) <= 1e-13 * want
    assert band[:, :, 1:-1].any() and not band[:, :, :2].any() and not band[:, :, -2:].any()      # interior nodes only
    I0, I1, I2 = LC.RAMP_I
    full = band.copy()
    full[3:5] = False
    assert np.array_equal(_bits(got[I_CW][full]), _bits(np.full(int(full.sum()), I0 + I1)))      # the mirrored pair shares a bin
    assert np.array_equal(_bits(got[I_SUM][full]), _bits(np.full(int(full.sum()), (I0 + I1) + I2)))
    assert np.array_equal(_bits(got[I_MAX][full]), _bits(np.full(int(full.sum()), I0)))
    assert (got[I_CW][3][band[3]] == I2).all() and (got[I_SUM][3][band[3]] == I2).all()         # beam 2 alone
    assert not got[1:4, 4].any() and not got[5:, 4].any() and (got[LN][4][band[4]] > 0).all()    # a band plane without light
    assert s["lit_cells"] == s["band_cells"] - int(band[4].sum()) and s["max_present"] == 3
    # the antiparallel beam sits in the LAST bin for every NB >= 2: with the pair's intensity lowered it is the common wave
    dim = c["fields"].copy()
    dim[0, :2] *= 0.25
    for nb in (2, 8, 16):
        alone, _ = _twin(api, c, fields=dim, cone_bins=nb)
        assert (alone[I_CW][full] == I2).all(), nb
    one, _ = _twin(api, c, fields=dim, cone_bins=1)
    assert np.array_equal(_bits(one[I_CW]), _bits(one[I_SUM]))


@pytest.mark.parametrize("name", ["traced", "crowded_wide"])
def test_exact_properties_of_the_model(api, cases, name):
    c = cases[name]
    got, s = _twin(api, c)
    one, s1 = _twin(api, c, cone_bins=1)
    assert np.array_equal(_bits(one[I_CW]), _bits(one[I_SUM])) and np.array_equal(_bits(one[ETA_CW]), _bits(one[ETA_SUM]))
    assert np.array_equal(_bits(one[[BAND, I_SUM, I_MAX, LN, ETA_SUM]]), _bits(got[[BAND, I_SUM, I_MAX, LN, ETA_SUM]]))
    assert s1["sum_I_cw"] == s1["sum_I_sum"] == s["sum_I_sum"]
    band = got[BAND] > 0
    assert (got[I_MAX] <= got[I_CW]).all() and (got[I_CW] <= got[I_SUM]).all()
    single = band & ((c["fields"][0] > 0).sum(axis=0) == 1)
    assert np.array_equal(_bits(got[I_CW][single]), _bits(got[I_SUM][single])) and np.array_equal(_bits(got[I_MAX][single]), _bits(got[I_SUM][single]))
    # fields x 2: a power of two scales every intensity, every sum of them and every eta exactly; L_n and the band do not move
    f2 = c["fields"].copy()
    f2[0] *= 2.0
    two, s2 = _twin(api, c, fields=f2)
    for q in (I_SUM, I_CW, I_MAX, ETA_SUM, ETA_CW):
        assert np.array_equal(_bits(two[q]), _bits(2.0 * got[q])), q
    assert np.array_equal(_bits(two[[BAND, LN]]), _bits(got[[BAND, LN]]))
    assert s2["sum_I_sum"] == 2.0 * s["sum_I_sum"] and s2["max_eta_cw"] == 2.0 * s["max_eta_cw"] and s2["argmax_cw"] == s["argmax_cw"]
    # a uniform te3d is the scalar path, bit for bit; te <= 0 in the table: eta = 0, the intensities stay
    uni, su = _twin(api, c, te=np.full(c["ne3d"].shape, 1234.5))
    sca, ss = _twin(api, c, te=1234.5)
    assert np.array_equal(_bits(uni), _bits(sca)) and su == ss
    cold, sc = _twin(api, c, te=np.zeros(c["ne3d"].shape))
    assert not cold[[ETA_SUM, ETA_CW]].any() and np.array_equal(_bits(cold[:5]), _bits(got[:5]))
    assert sc["max_eta_cw"] == 0.0 and sc["above_sum"] == 0 and sc["band_cells"] == s["band_cells"] and sc["argmax_cw"] == int(np.flatnonzero(band.reshape(-1))[0])
    # the summary is the stack's
    flat = np.flatnonzero(band.reshape(-1))
    assert s["band_cells"] == flat.size and s["argmax_cw"] == int(flat[np.argmax(got[ETA_CW].reshape(-1)[flat])])
    assert s["max_eta_cw"] == got[ETA_CW].max() and s["max_eta_sum"] == got[ETA_SUM].max()
    assert s["above_cw"] == int((got[ETA_CW] >= 1).sum()) and s["above_sum"] == int((got[ETA_SUM] >= 1).sum())


def test_bands_slabs_and_merging(api, cases):
    c = cases["traced"]
    whole, s = _twin(api, c)
    # an empty band: all zeros, argmax_cw = -1
    none, s0 = _twin(api, c, band=(0.999, 0.999))
    assert not none.any() and s0["argmax_cw"] == -1 and s0["band_cells"] == 0 and s0["max_eta_cw"] == 0.0
    # frac_lo == frac_hi works: exactly the nodes with that density
    node = c["ne3d"][24, 10, 40]
    frac = float(node / api.derive(c["p"]).ncrit)
    point, sp = _twin(api, c, band=(frac, frac))
    assert sp["band_cells"] == int((LC.halo(c["ne3d"]) == node).sum()) >= 1
    # slab calls write their planes only and merge into one summary: the whole call's stack and counts, sums to the last bits
    from helpers.gain_worlds import CUTS
    out = np.full(whole.shape, -7.0)
    merged = api.lpi_summary_new()
    for lo, hi in zip(CUTS["traced"][:-1], CUTS["traced"][1:]):
        before = out.copy()
        api.lpi_map_host(c["fields"], c["ne3d"], c["p"], te=c["te"], band=c["band"], cone_bins=c["nbins"], hx_lo=lo, hx_hi=hi, out=out, summary=merged)
        assert np.array_equal(out[:, :lo], before[:, :lo]) and np.array_equal(out[:, hi:], before[:, hi:])
    assert np.array_equal(_bits(out), _bits(whole))
    m = merged.as_dict()
    for k in LC.COUNTS + LC.MAXIMA:
        assert m[k] == s[k], k
    for k, q in zip(LC.SUMS, (I_SUM, I_CW)):
        assert abs(m[k] - s[k]) <= LC.any_order_bound(whole[q][whole[BAND] > 0]), k


def test_three_node_axis_is_all_faces(api):
    """The smallest axis the library takes: every node of it differences nodes 0 and 2 (the 2-node axis of the header's guard
    is walked by tests/test_lpi_sanitizers.py: the entries refuse such a grid)."""
    from helpers import gain_worlds as W
    p = W.params(api, (5, 3, 6), 2)
    d = api.derive(p)
    rng = np.random.default_rng(5)
    ne3d = d.ncrit * (0.2 + 0.05 * rng.random((5, 3, 6)))
    fields = np.zeros((4, 2, 7, 5, 8))
    fields[0], fields[3, 0], fields[2, 1] = 1e14, 1.0e5, -1.0e5
    got, s = api.lpi_map_host(fields, ne3d, p, te=1500.0)
    ref, rs, near = LC.lpi_reference(api, p, fields, ne3d, 1500.0)
    assert s["band_cells"] == 7 * 5 * 8 == rs["band_cells"] and not near.any()
    assert np.allclose(got, ref, rtol=LAST_BITS, atol=0.0)
    gy = (ne3d[:, 2] - ne3d[:, 0]) / (2.0 * d.dy)                  # the same for all three nodes of the axis
    assert gy.any()


# ---- the derived quantities -------------------------------------------------------------------------------------------------
def test_srs_parameter_and_summarize(api):
    from cbet_raytracing_3d_amd import lpi
    lam = 0.351
    L_um = 2377.0 ** 0.75 / lam ** 0.5                          # I_14 = 1: L^(4/3) lambda^(2/3) = 2377
    assert abs(lpi.srs_parameter(1e14, L_um * 1e-4, lam) - 1.0) < 1e-14
    assert abs(lpi.srs_parameter(np.array([2e14, 0.0]), np.array([L_um * 1e-4, 1.0]), lam) - np.array([2.0, 0.0])).max() < 1e-13
    assert lpi.srs_parameter(3e14, 0.0, lam) == 0.0
    assert abs(lpi.wavelength_um(api.default_params(16)) - 0.351) < 1e-3
    s = dict(api.lpi_summary_new().as_dict(), band_cells=8, lit_cells=6, above_max=1, above_cw=2, above_sum=4, sum_I_sum=16e14,
             sum_I_cw=8e14, max_eta_cw=1.5, argmax_cw=77, max_present=3)
    out = lpi.summarize(s)
    assert out["lit_fraction"] == 0.75 and out["above_cw_fraction"] == 0.25 and out["above_sum_fraction"] == 0.5
    assert out["mean_I_sum"] == 2e14 and out["mean_I_cw"] == 1e14 and out["max_eta_cw"] == 1.5 and out["argmax_cw"] == 77
    empty = lpi.summarize(api.lpi_summary_new().as_dict())
    assert empty["band_cells"] == 0 and np.isnan(empty["mean_I_sum"]) and empty["argmax_cw"] == -1
