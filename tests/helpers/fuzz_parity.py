"""Randomised parity sweep on the GPU: small random grids (ragged, tiny, face-hugging), beam subsets, rays per
zone, absorption on/off, sharding, beam-resolved grids, all three kernel formulations -- every case against
the CPU oracle (SURVEY 8(c) metric <= 1e-9, equal ray-step counts).
usage: python tests/helpers/fuzz_parity.py [cases=40] [seed=1] [knobs=0] [oracle]

knobs=1: a SEPARATE generator (so that knobs=0 draws exactly the cases it always drew) adds per plain case a Courant
multiplier, six independently moved box bounds, a launch rule (threads_per_block, max_threads) and beam rows that
are random unit vectors or +-axes instead of OMEGA rows.  A case whose ORACLE output is not finite (the reference's own
NaN, see the n >= 4 note below) is skipped; the share of skipped cases is printed and must stay <= 10 %.
oracle: the draw and the oracle half only -- no GPU is touched; reports the skipped share for a seed."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_inputs, parity_err
from cbet_raytracing_3d_amd import api
from oracle import cbet_oracle as O
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
knobs = len(sys.argv) > 3 and sys.argv[3] not in ("0", "off", "")
oracle_only = len(sys.argv) > 4 and sys.argv[4] == "oracle"
if not oracle_only:
    import torch
    from cbet_raytracing_3d_amd.tracer import RayTracer
rng = np.random.default_rng(seed)
krng = np.random.default_rng([seed, 0x6B6E6F62])      # the knobs' own stream
bn, r, ne, te = load_inputs()
COURANTS = (0.25, 0.5, 0.8, 1.0, 1.3, 1.7, 2.5)
BOUNDS = ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")


def draw_knobs(nb, rows):
    """(overrides for cbet_params and the oracle's config alike, beam rows)."""
    kn = {"courant_mult": float(krng.choice(COURANTS))}
    for name in BOUNDS:      # each bound on its own, by up to +-40 % of the half-width: max > min always holds
        kn[name] = (-0.13 if name.endswith("min") else 0.13) + 0.4 * 0.13 * float(krng.uniform(-1.0, 1.0))
    kn["threads_per_block"] = int(krng.choice([7, 64, 96, 256, 1000]))
    if krng.random() < 0.5:
        kn["max_threads"] = nb * int(krng.integers(500, 5001))
    rows = rows.copy()
    for b in range(nb):
        if krng.random() < 0.3:
            if krng.random() < 0.5:
                v = krng.standard_normal(3)
                rows[b] = v / np.linalg.norm(v)
            else:
                rows[b] = 0.0
                rows[b, int(krng.integers(3))] = float(krng.choice([-1.0, 1.0]))
    return kn, rows


skipped = 0
worst, bad = 0.0, 0
for case in range(cases):
    # n >= 4 per axis: with 3 nodes the launch plane (focal length - dz/2) lies inside the over-critical core and
    # the dispersion relation yields NaN wave vectors -- in the reference's formulas as much as here
    nx, ny, nz = (int(v) for v in rng.integers(4, 56, size=3))
    if rng.random() < 0.3: ny = nz = nx
    rpz = int(rng.integers(1, 7))
    nb = int(rng.integers(1, 7))
    beams = sorted(rng.choice(60, size=nb, replace=False).tolist())
    absorb = int(rng.random() < 0.8)
    variant = int(rng.choice([0, 1, 2, 3]))
    kw = {}
    wide = int(rng.random() < 0.2)
    shards = int(rng.choice([1, 1, 2, 3]))
    per_beam = bool(rng.random() < 0.3)
    p = api.default_params(nx, nbeams=nb, rays_per_zone=rpz, absorption=absorb, kernel_variant=variant, force_wide_index=wide)
    p.ny, p.nz = ny, nz
    desc = dict(grid=(nx, ny, nz), rpz=rpz, beams=beams, absorption=absorb, variant=variant, knobs=kw, wide=wide, shards=shards, per_beam=per_beam)
    rows, kn = bn[beams].copy(), {}
    if knobs:
        kn, rows = draw_knobs(nb, rows)
        for k, v in kn.items():
            setattr(p, k, v)
        desc.update(kn, rows=rows.tolist())
    try:
        if oracle_only:
            tr = None
            api.derive(p)
        else:
            tr = RayTracer(p, r, ne, te, beam_norm=rows)
    except api.CbetError as exc:
        skipped += 1
        print("case %d skipped (%s): %s" % (case, exc, desc)); continue
    # a third of the single-grid cases deposit into a grid with padded rows (cbet_params.edep_zpitch)
    zpitch = int(nz + 2 + rng.integers(1, 10)) if (not per_beam and rng.random() < 0.33) else None
    desc["zpitch"] = zpitch
    cfg = O.default_config(nx, nbeams=nb, rays_per_zone=rpz, absorption=absorb, **kn)
    cfg.ny, cfg.nz = ny, nz
    if per_beam:
        want, osteps = [], 0
        for b in range(nb):
            ob, st = O.trace(cfg, rows.copy(), r, ne, te, beam_lo=b, beam_hi=b + 1, nthreads=8)
            osteps += st
            want.append(ob)
    else:
        oe, osteps = O.trace(cfg, rows.copy(), r, ne, te, nthreads=8)
        want = [oe]
    if not all(np.isfinite(w).all() for w in want):      # the reference's own NaN: not a case (and never shown to a kernel)
        skipped += 1
        print("case %2d skipped (oracle output not finite): %s" % (case, desc), flush=True)
        if tr is not None:
            tr.close()
        continue
    if oracle_only:
        print("case %2d oracle ok, steps %d" % (case, osteps), flush=True)
        continue
    e = tr.new_grid(per_beam=per_beam, zpitch=zpitch)
    tr.counters(reset=True)
    for s in range(shards):
        tr.launch(e, shard_index=s, shard_count=shards, **kw)
    c = tr.counters(reset=True)
    got = e.cpu().numpy()
    if zpitch:
        pad_clean = bool((got[..., nz + 2:] == 0).all())     # the padding is never touched
        got = got[..., : nz + 2]
    else:
        pad_clean = True
    if per_beam:
        err = max(parity_err(got[b], ob) if np.abs(ob).max() > 0 else float(np.abs(got[b]).max()) for b, ob in enumerate(want))
    else:
        err = parity_err(got, oe) if np.abs(oe).max() > 0 else float(np.abs(got).max())
    ok = err < 1e-9 and c.ray_steps == osteps and pad_clean
    worst = max(worst, err)
    bad += not ok
    print("case %2d %s err %.2e steps %d/%d %s" % (case, "ok  " if ok else "FAIL", err, c.ray_steps, osteps, "" if ok else desc), flush=True)
    tr.close()
share = skipped / max(1, cases)
print("skipped %d of %d cases (%.1f %%)" % (skipped, cases, 100.0 * share))
if share > 0.10:
    print("too many skipped cases: the sweep no longer tests what it draws")
    sys.exit(1)
if oracle_only:
    sys.exit(0)
# the CBET hooks (parity unpinned: checked against the CPU restatement of the model): fused field pass,
# gain kernels and deposition pass with a random gain field on random small grids
gp, og = api.default_gain_params(relax=1.0), O.gain_default()
for case in range(max(4, cases // 5)):
    nx, ny, nz = (int(v) for v in rng.integers(4, 40, size=3))
    rpz = int(rng.integers(2, 6))
    nb = int(rng.integers(2, 6))
    beams = sorted(rng.choice(60, size=nb, replace=False).tolist())
    p = api.default_params(nx, nbeams=nb, rays_per_zone=rpz, force_wide_index=int(rng.random() < 0.2))
    p.ny, p.nz = ny, nz
    tr = RayTracer(p, r, ne, te, beam_norm=bn[beams])
    tr.tabulate()
    cfg = O.default_config(nx, nbeams=nb, rays_per_zone=rpz)
    cfg.ny, cfg.nz = ny, nz
    ne3d, kap = O.node_tables(cfg, r, ne, te)
    gain = rng.uniform(-60.0, 60.0, size=(nb, nx + 2, ny + 2, nz + 2))
    d_gain = torch.from_numpy(gain).cuda()
    f, e = tr.new_fields(), tr.new_grid()
    bg = torch.zeros(nb, dtype=torch.float64, device="cuda")
    tr.launch_cbet(f, gp, fields=True, gain=d_gain)
    tr.launch_cbet(e, gp, gain=d_gain, beam_gain=bg)
    fe = tr.new_fields()
    tr.launch_cbet(fe[0], gp, fields="energy", gain=d_gain)     # the energy field alone, z-brick kernel
    of = np.stack([O.trace_cbet(cfg, og, bn[beams].copy(), ne3d, kap, gain=gain, quantity=q, per_beam=True, nthreads=8)[0]
                   for q in (1, 2, 3, 4)])
    oe, osteps, obg = O.trace_cbet(cfg, og, bn[beams].copy(), ne3d, kap, gain=gain, nthreads=8)
    errs = [float(np.abs(f.cpu().numpy() - of).max() / max(np.abs(of).max(), 1e-300)),
            float(np.abs(fe[0].cpu().numpy() - of[0]).max() / max(np.abs(of[0]).max(), 1e-300)),
            parity_err(e.cpu().numpy(), oe) if np.abs(oe).max() > 0 else 0.0,
            float(np.abs(bg.cpu().numpy() - obg).max() / max(np.abs(obg).max(), 1e-300))]
    K = {}
    for sym in (False, True):      # both gain kernels on the oracle's fields
        g2 = tr.new_grid(per_beam=True)
        df = torch.from_numpy(of.copy()).cuda()
        tr.gain_field(df, g2, gp, None, scratch=torch.empty_like(g2) if sym else None)
        K[sym] = g2.cpu().numpy()
        # ... and again with fresh energy on top of the direction entries that call left (frozen directions)
        df[0] = torch.from_numpy(of[0].copy()).cuda()
        g3 = tr.new_grid(per_beam=True)
        tr.gain_field(df, g3, gp, None, scratch=torch.empty_like(g3) if sym else None, frozen=True)
        K[(sym, "frozen")] = g3.cpu().numpy()
    ok_, _ = O.gain_field(cfg, og, of, ne3d, relax=1.0, nthreads=8)
    scale = max(np.abs(ok_).max(), 1e-300)
    errs += [float(np.abs(K[False] - ok_).max() / scale), float(np.abs(K[True] - ok_).max() / scale),
             float(np.abs(K[(False, "frozen")] - ok_).max() / scale), float(np.abs(K[(True, "frozen")] - ok_).max() / scale)]
    ok = max(errs) < 1e-9
    worst = max(worst, max(errs)); bad += not ok
    print("cbet case %2d %s grid %s beams %d rpz %d: fields %.1e energy field %.1e edep %.1e beam-gain %.1e K %.1e K(sym) %.1e frozen %.1e %.1e (max |K| %.3g)" %
          ((case, "ok  " if ok else "FAIL", (nx, ny, nz), nb, rpz) + tuple(errs) + (float(np.abs(ok_).max()),)), flush=True)
    tr.close()
print("cases %d, failures %d, worst err %.2e" % (cases, bad, worst))
sys.exit(1 if bad else 0)
