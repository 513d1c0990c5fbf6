"""Host-side checks of the C-ABI library that need no GPU: it loads, exports every symbol the
header declares, and its host arithmetic (derived constants, tables, launch list, error paths)
agrees with the oracle to the last bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import DATA, ROOT
from helpers import config_matrix as M


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


def test_library_exports_every_declared_symbol(api):
    hdr = open(os.path.join(ROOT, "include", "cbet_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cbet_[A-Za-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(api.EXPORTS)
    L = C.CDLL(api.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(L, name), name


_C_KINDS = {"int": "int", "unsigned": "unsigned", "unsigned int": "unsigned", "long": "i64", "long long": "i64",
            "size_t": "u64", "unsigned long long": "u64", "double": "double", "void": "void", "char": "char"}


def _c_kind(ctype):
    """(kind, pointee) of a C type without its parameter name: anything with * or [ is a pointer, whose pointee is the type
    with one * or [n] taken off; kind None = not classified."""
    t = " ".join(re.sub(r"\bconst\b", " ", ctype).split())
    if "*" in t or "[" in t:
        return "ptr", re.sub(r"\s*(\*|\[\d*\])$", "", t, count=1).strip()
    return _C_KINDS.get(t), None


def _ctypes_kind(ct):
    if ct is None:
        return "void"
    if ct in (C.c_void_p, C.c_char_p) or issubclass(ct, C._Pointer):
        return "ptr"
    return {C.c_int: "int", C.c_uint: "unsigned", C.c_long: "i64", C.c_longlong: "i64", C.c_size_t: "u64",
            C.c_ulonglong: "u64", C.c_double: "double"}.get(ct)


def _mismatch(api, ctype, ct):
    """Why the ctypes type `ct` does not describe the C type `ctype`, or None if it does."""
    kind, pointee = _c_kind(ctype)
    if kind is None:
        return "the C type %r is not classified" % ctype
    if kind != _ctypes_kind(ct):
        return "%r is %s in the header, %s in the table" % (ctype, kind, _ctypes_kind(ct))
    if kind == "ptr" and (ct is C.c_char_p or pointee == "char"):
        return None if (ct is C.c_char_p and pointee == "char") else "%r and c_char_p go together" % ctype
    if kind == "ptr" and ct is not C.c_void_p:              # POINTER(T): the header's pointee is T
        target = ct._type_
        if issubclass(target, C.Structure):
            names = [name for name, cls in api.STRUCTS.items() if cls is target]
            return None if names == [pointee] else "%r points to %s in the table" % (ctype, names or target.__name__)
        if _c_kind(pointee)[0] != _ctypes_kind(target):
            return "%r points to %s in the table" % (ctype, target.__name__)
    return None


def test_signatures_match_header(api):
    """api.SIGNATURES vs the prototypes of the C header: the same names, and the return type and every parameter of the same
    kind -- pointer, int, unsigned, signed or unsigned 64-bit, double, void; a POINTER(T) of the table points to the
    header's T (a struct by its name in api.STRUCTS), and char * is c_char_p."""
    hdr = open(os.path.join(ROOT, "include", "cbet_mi355x.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    protos = {m.group(2): (m.group(1), m.group(3))
              for m in re.finditer(r"^[ \t]*([\w \t\*]+?)\b(cbet_\w+)[ \t]*\(([^()]*)\)\s*;", hdr, flags=re.M)}
    assert set(protos) == set(api.SIGNATURES), sorted(set(protos) ^ set(api.SIGNATURES))
    errors = []
    for name, (ret, params) in protos.items():
        restype, argtypes = api.SIGNATURES[name]
        params = [] if params.strip() == "void" else [re.sub(r"\w+\s*(\[\d*\])?\s*$", r"\1", p.strip()) for p in params.split(",")]
        if len(params) != len(argtypes):
            errors.append("%s: %d parameters in the header, %d in the table" % (name, len(params), len(argtypes)))
            continue
        for where, ctype, ct in [("return", ret, restype)] + [("argument %d" % k, c, t) for k, (c, t) in enumerate(zip(params, argtypes))]:
            why = _mismatch(api, ctype, ct)
            if why:
                errors.append("%s, %s: %s" % (name, where, why))
    assert not errors, "\n".join(errors)
    L = api.lib()
    for name, (restype, argtypes) in api.SIGNATURES.items():      # ... and the table is what the loaded library is called by
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == list(argtypes), name


def test_struct_layout_matches_header(api, tmp_path):
    """ctypes mirrors vs the C header: sizeof and every field offset of every struct of api.STRUCTS, asked of gcc; the numpy
    dtypes of the four records have the same size and offsets."""
    import subprocess
    probes = api.STRUCTS
    assert len(probes) == 14
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cbet_mi355x.h"', 'int main(void){']
    for cname, cls in probes.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    for cname, cls in probes.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, fname)]) == getattr(cls, fname).offset, (cname, fname)
    twins = {"cbet_ray_exit": api.EXIT_DTYPE, "cbet_path_sample": api.PATH_DTYPE, "cbet_ray_turn": api.TURN_DTYPE,
             "cbet_ray_sbs": api.SBS_DTYPE}
    for cname, dt in twins.items():
        assert dt.itemsize == int(got[cname]) and dt.names == tuple(f for f, _ in probes[cname]._fields_), cname
        for fname in dt.names:
            assert dt.fields[fname][1] == int(got["%s.%s" % (cname, fname)]), (cname, fname)
            assert dt.fields[fname][0].itemsize == C.sizeof(dict(probes[cname]._fields_)[fname]), (cname, fname)
    p = api.default_params(100)
    assert (p.nx, p.nbeams, p.rays_per_zone, p.nprofile, p.max_threads, p.threads_per_block) == \
        (100, 60, 4, 443, 120000000, 256)
    assert (p.xmin, p.xmax, p.courant_mult, p.absorption) == (-0.13, 0.13, 0.5, 1)


@pytest.mark.parametrize("n", [64, 100, 256, 512] + M.ENTRIES, ids=str)
def test_derived_bitwise_equal_to_oracle(api, oracle, n):
    """The default configuration at four sizes, then every entry of the configuration matrix (Courant, box, launch rule)."""
    if isinstance(n, M.Entry):
        d, o = api.derive(n.params(api)), oracle.derive(n.config(oracle))
    else:
        d = api.derive(api.default_params(n))
        o = oracle.derive(oracle.default_config(n))
    for f in ("dx", "dy", "dz", "dt", "nt", "zones_spanned", "nrays_x", "nrays_y", "nrays", "omega",
              "ncrit", "uray_mult", "xconst", "yconst", "zconst", "threads_per_beam", "nindices",
              "grid_y", "edep_size"):
        assert getattr(d, f) == getattr(o, f), f


def test_host_tables_bitwise_equal_to_oracle(api, oracle, inputs):
    bn = inputs[0]
    ph, pw = api.host_power_table()
    oph, opw = oracle.power_table()
    assert np.array_equal(ph, oph) and np.array_equal(pw, opw)
    assert np.array_equal(api.host_beam_trig(bn), oracle.beam_trig(bn))


def test_beam_table_and_profiles(api, inputs):
    bn, r, ne, te = inputs
    assert np.array_equal(api.omega60_beam_norm(), bn)
    assert np.allclose(np.linalg.norm(bn, axis=1), 1.0, atol=1e-8)
    r2, ne2, te2 = api.load_s83177()
    assert np.array_equal(r2, r) and np.array_equal(ne2, ne) and np.array_equal(te2, te)
    # exactly 443 rows are read (def.cuh:33); the file's 444th row (r=0.343967, 0) is never used
    assert len(open(os.path.join(DATA, "s83177_ne.txt")).read().split()) == 888
    with pytest.raises(api.CbetError) as ei:
        api.read_profile(os.path.join(DATA, "s83177_ne.txt"), 445)
    assert ei.value.code == api.EINVAL


@pytest.mark.parametrize("n", [64, 100] + M.ENTRIES, ids=str)
def test_live_list_is_the_reference_ray_set(api, oracle, inputs, n):
    bn = inputs[0]
    if isinstance(n, M.Entry):      # a matrix entry: its own box, launch rule and beam table (beam 0 of it)
        p, cfg, bt = n.params(api), n.config(oracle), n.beam_table(bn)
        slots = api.live_ray_list(p)
        live = slots[slots >= 0]
        d = api.derive(p)
        assert len(slots) % 64 == 0 and all((slots[k:k + 64] >= 0).any() for k in range(0, len(slots), 64))
        assert len(live) == d.nlive_rays and len(set(live.tolist())) == len(live)
        assert sorted(live.tolist()) == M.live_ids(oracle, cfg, bt)
        return
    p = api.default_params(n)
    slots = api.live_ray_list(p)
    live = slots[slots >= 0]
    d = api.derive(p)
    assert len(slots) % 64 == 0 and all((slots[k:k + 64] >= 0).any() for k in range(0, len(slots), 64))
    assert len(live) == d.nlive_rays and len(set(live.tolist())) == len(live)
    cfg = oracle.default_config(n)
    L = oracle.lib()
    want = [i for i in range(d.nrays)
            if L.cbet_oracle_id_is_traced(C.byref(cfg), i) and oracle.launch_point(cfg, bn, 7, i)[0]]
    assert sorted(live.tolist()) == want
    if n == 100:
        assert len(live) == 15102 and d.ntraced_ids == 19456


@pytest.mark.parametrize("entry", M.ENTRIES, ids=str)
def test_matrix_entry_reaches_its_regime(oracle, inputs, entry):
    """Each entry of the configuration matrix is named for a regime (rays lost after a far jump, rays launched outside
    the box, strided passes, ...): assert from the oracle's ray paths of a seeded sample that it still gets there, and
    that its ray-step count is the one recorded when the table was written."""
    st = M.regime_stats(oracle, entry, inputs)
    print(st)
    assert st["unit_beams"] and st["nlive"] > 0
    entry.regime(st)
    if entry.name in M.PINNED_STEPS:
        assert M.oracle_trace(oracle, entry, inputs)[1] == M.PINNED_STEPS[entry.name]


def test_bundles_are_compact_patches(api, oracle, inputs):
    """One bundle = an 8x8-ray patch: its launch points span at most 2 cells in-plane, and only patches on the rim of
    the beam have holes.  With cbet_params.rim_merge (default 4 launch zones = 16 rays) the rays of the rim patches are packed into full bundles:
    the same rays, fewer bundles, fewer idle lanes, a footprint of at most 16 rays = 4 cells."""
    bn = inputs[0]
    cfg = oracle.default_config(256)

    def spans(p, slots, picks):
        d = api.derive(p)
        out = []
        for k in picks:
            ids = slots[k:k + 64]
            pts = np.array([oracle.launch_point(cfg, bn, 11, int(i))[1][:3] for i in ids[ids >= 0]])
            out.append(np.ptp(pts, axis=0).max() / d.dx)
        return out

    p0 = api.default_params(256, rim_merge=0)
    d = api.derive(p0)
    s0 = api.live_ray_list(p0)
    fill0 = (s0.reshape(-1, 64) >= 0).sum(1)
    assert len(fill0) == 1620 and (fill0 == 64).mean() > 0.9 and fill0.sum() == d.nlive_rays == 98872
    assert d.nlive_rays / len(s0) > 0.95           # idle lanes from holes: < 5 %
    assert max(spans(p0, s0, (0, 640, 64 * 700, len(s0) - 64))) <= 2.0 * 1.0001
    p = api.default_params(256)
    assert p.rim_merge == 4
    s = api.live_ray_list(p)
    fill = (s.reshape(-1, 64) >= 0).sum(1)
    assert sorted(s[s >= 0].tolist()) == sorted(s0[s0 >= 0].tolist())          # the same rays, each once
    assert len(fill) < 1560 and d.nlive_rays / len(s) > 0.99 and (fill < 64).sum() < 40
    partial = [64 * int(k) for k in np.nonzero(fill < 64)[0][:6]] + [64 * int(k) for k in np.argsort(-fill)[:2]]
    merged = [64 * int(k) for k in range(len(fill)) if len(set((s[64 * k:64 * k + 64][s[64 * k:64 * k + 64] >= 0] // 16).tolist())) > 4][:8]
    assert merged                                                                # bundles that hold rays of more than 4 zones
    assert max(spans(p, s, partial + merged)) <= 4.0 * 1.0001
    # the order of the full patches is untouched: the full bundles appear in the same sequence
    full0 = [tuple(b) for b in s0.reshape(-1, 64) if (b >= 0).all()]
    full = [tuple(b) for b in s.reshape(-1, 64) if tuple(b) in set(full0)]
    assert full == full0
    with pytest.raises(api.CbetError):
        api.live_ray_list(api.default_params(64, rim_merge=1))


def test_shard_plan_partitions_the_work(api):
    p = api.default_params(64)
    nb = 3
    full_b, full_i = api.shard_items(p, nb, 0, 1)
    assert len(full_i) == nb * api.derive(p).nlive_rays
    seen = []
    for s in range(4):
        b, i = api.shard_items(p, nb, s, 4)
        seen.append(np.stack([b, i], 1))
    allp = np.concatenate(seen)
    assert len(allp) == len(full_i)
    assert len({(int(a), int(b)) for a, b in allp}) == len(full_i)
    # contiguous parts of the beam-major list: each shard's beams form a contiguous run, the shards are in list order
    # and hold the same number of bundles to within one
    bpb = (len(api.live_ray_list(p)) + 63) // 64
    firsts = [int(s[0, 0]) for s in seen]
    assert firsts == sorted(firsts) and all(np.all(np.diff(s[:, 0]) >= 0) for s in seen)
    live = api.live_ray_list(p)
    per_bundle = (live.reshape(-1, 64) >= 0).sum(1)
    tiled = np.tile(per_bundle, nb)
    T = nb * bpb
    assert [len(s) for s in seen] == [int(tiled[(k * T) // 4:((k + 1) * T) // 4].sum()) for k in range(4)]


def test_error_paths_without_a_gpu(api):
    p = api.default_params(100)
    bad = p.copy(nx=2)
    with pytest.raises(api.CbetError) as ei:
        api.derive(bad)
    assert ei.value.code == api.EINVAL
    with pytest.raises(api.CbetError) as ei:
        api.derive(p.copy(shard_count=4, shard_index=4))
    assert ei.value.code == api.EINVAL
    with pytest.raises(api.CbetError) as ei:
        api.derive(p.copy(nx=1400, ny=1400, nz=1400))   # (n+2)^3 >= 2^31: 32-bit node tags
    assert ei.value.code == api.EINVAL
    # thin anisotropic grids: the kernels form cell and node indices with 24-bit multiplies, so nx*ny and
    # (ny+2)(nz+2) must stay below 2^23 even when the whole grid is far below 2^31 nodes
    for shape in (dict(nx=4000, ny=4000, nz=3), dict(nx=200, ny=3000, nz=3000), dict(nx=3, ny=2900, nz=2900)):
        with pytest.raises(api.CbetError) as ei:
            api.derive(p.copy(**shape))
        assert ei.value.code == api.EINVAL and "anisotropic" in str(ei.value)
    api.derive(p.copy(nx=2800, ny=2900, nz=3))         # 8.1e6 < 2^23 = 8.4e6: accepted
    # a padded row pitch of the caller's deposit grid: 0 (dense) or at least nz + 2
    api.derive(p.copy(edep_zpitch=104))
    for bad_pitch in (101, -8, 1 << 22):
        with pytest.raises(api.CbetError) as ei:
            api.derive(p.copy(edep_zpitch=bad_pitch))
        assert ei.value.code == api.EINVAL and "edep_zpitch" in str(ei.value)
    with pytest.raises(api.CbetError) as ei:           # multi_gpu.cpp:45-48
        api.moveToAndFromGPU(np.zeros(4), np.zeros(4), 32, -1)
    assert ei.value.code == api.ENODEVICE


def test_product_does_not_import_the_oracle():
    """The shipped path must never route through oracle/ (only tests, smoke and the bench's
    cpu_baseline leg may)."""
    pkg = os.path.join(ROOT, "cbet_raytracing_3d_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "cbet_oracle" not in text and "import oracle" not in text, f


def test_text_writer_matches_reference_format(api, oracle, inputs, tmp_path):
    """cbet_write_text (main.cu:6-22): byte-identical to the oracle's writer on awkward values, and
    the md5 the survey's host compile of the reference kernel recorded for the 100^3 dump (never compared
    with truth_100, which is absent from the mount) when fed the oracle's 100^3 grid -- the reference's `make test`
    criterion, Makefile:14-17."""
    import hashlib
    rng = np.random.default_rng(5)
    a = rng.standard_normal((3, 4, 5)) * 10.0 ** rng.integers(-8, 14, (3, 4, 5))
    a[0, 0, 0], a[1, 2, 3], a[2, 3, 4], a[0, 1, 1] = 0.0, -0.0, 1e6, 123456.5
    p1, p2 = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    n1, n2 = api.write_text(a, p1), oracle.write_text(a, p2)
    assert n1 == n2 == os.path.getsize(p1)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    assert open(p1).read().startswith("[[[") and open(p1).read().endswith("]\n]\n]\n")
    bn, r, ne, te = inputs
    e, _ = oracle.trace(oracle.default_config(100), bn, r, ne, te, nthreads=os.cpu_count())
    p3 = str(tmp_path / "truth.txt")
    assert api.write_text(e, p3) == 12544620
    assert hashlib.md5(open(p3, "rb").read()).hexdigest() == "cc0909ed1c5938704c51165dc20cb829"


def test_edep_average(api):
    rng = np.random.default_rng(7)
    e = rng.uniform(0, 1e12, (7, 9, 8))
    got = api.edep_average(e)
    assert got.shape == (5, 7, 6)
    want = np.zeros_like(got)
    for di in range(3):
        for dj in range(3):
            for dk in range(3):
                want += e[di:di + 5, dj:dj + 7, dk:dk + 6]
    assert np.allclose(got, want / 27, rtol=1e-14, atol=0)
    # literal order of main.cu:338-346 for one cell: k-offset outermost, then j, then i
    acc = None
    for dk in range(3):
        for dj in range(3):
            for di in range(3):
                v = e[2 + di, 3 + dj, 1 + dk]
                acc = v if acc is None else acc + v
    assert got[2, 3, 1] == acc / 27


def test_npy_writer_and_node_coordinates(api, tmp_path):
    """The .npy stand-in for the reference's (dead) HDF5 output: numpy must read back what the library wrote,
    for shapes whose header lengths exercise the 64-byte padding; coordinates as main.cu:321-332."""
    rng = np.random.default_rng(3)
    for shape in ((7,), (3, 4), (2, 3, 5), (11, 1, 13), (1, 1, 1, 2), (100000,)):
        a = rng.standard_normal(shape)
        path = tmp_path / ("a_%s.npy" % "x".join(map(str, shape)))
        n = api.write_npy(a, str(path))
        assert n == os.path.getsize(path) and (n - a.nbytes) % 64 == 0
        b = np.load(path)
        assert b.dtype == np.float64 and b.shape == shape and np.array_equal(a, b) and b.flags["C_CONTIGUOUS"]
    with pytest.raises(api.CbetError):
        api.write_npy(np.zeros(3), str(tmp_path / "no_such_dir" / "a.npy"))
    p = api.default_params(6)
    p.ny, p.nz = 4, 5
    x, y, z = api.node_coordinates(p)
    d = api.derive(p)
    assert x.shape == (6, 4, 5)
    assert np.array_equal(x[:, 2, 3], np.arange(6) * d.dx + p.xmin) and np.array_equal(y[1, :, 0], np.arange(4) * d.dy + p.ymin)
    assert np.array_equal(z[5, 3, :], np.arange(5) * d.dz + p.zmin)
