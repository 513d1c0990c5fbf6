"""The designed pair cases of tests/test_pair_accuracy_host.py and tests/test_gpu_pair_accuracy.py (DESIGN.md section 9,
"Per-pair accuracy"): one case per node of a 4 x 3 x 148 grid, two worlds on it, and the 200-bit model they are judged by.

The grid.  Haloed 6 x 5 x 150: rows of 150 cells, three 64-cell state groups with a last group of 22 cells, rows that start off a
128-byte line -- CROWDED's z shape (helpers/gain_worlds.py), the smallest that reaches every run arm.  Halo cells hold E = 0 for
every beam.  Every input is a double chosen here: ne per node, a caller's flow table, a state table (cs, gain_const), the beams'
k vectors and energies written into the fields; the kernels are called FROZEN, so k is read as it is and only I = E / ds is formed.
k is built as the kernels' own normalisation builds it, kmag (a / |a|) with one rounding per operator.

The cases (build_inputs): crossing angle x eta x construction crossed in full, the density cycling so that every (eta, frac) and
(angle, frac) combination occurs; then pairs one ulp apart in one component, nodes at and above critical density, one beam absent
(E = 0 or E < 0), two exactly parallel beams of different colour (q = 0, dw != 0).  Constructions of eta = N / D:
  along          u along q:  N = -(q . u) has one sign in all three products
  perpendicular  u = 4e7 p + s q with p perpendicular to q: the three products of q . u cancel
  beat           u random, eta set through the beat frequency dw = w_j - w_i: the designed eta holds in the DETUNE sets
World A has two beams (every cell one isolated pair), world B sixty with three present per cell: A's pair and a third beam at
another designed angle, the beam numbers rotating along z so that 16-cell runs hold <= 20, 21 - 40 and > 40 present beams.

The model (model): mpmath at 200 bits, sharing no line with the library or with helpers/gain_reference.py.  From the doubles:
    frac = ne / ncrit, eps = 1 - frac, I = E / ((c sqrt(eps)) dt), q = k_j - k_i, D = |q| cs + 1e-10, N = -(q . u) (+ dw)
    P(eta) = iaw^2 eta / ((eta^2 - 1)^2 + iaw^2 eta^2),  G_ij = pref P(N / D),  pref = gain_const frac (1 / iaw) / sqrt(eps)
    BAND: G_ij = pref sum_a sum_b p_a p_b P((N + (o_b - o_a)) / D)      POL: G_ij times (1 + cth^2) / 4, cth = k_i . k_j / kmag^2
    SAT: G_ij scaled by lim / w where w = |G_ij| sqrt(Ii Ij) > lim = dn_max (k0 / 2) frac / sqrt(eps)
    K_i = sum_j G_ij I_j
and beside it the scale S_i, the first-order sensitivity of K_i to one rounding of each cancelling addend:
    S_i = sum_j [ |G_ij I_j| (1 + frac / eps) + I_j |pref P'(eta_ij)| / D (|q_x u_x| + |q_y u_y| + |q_z u_z| + |dw| (+ |o_b - o_a|)) ]
the first term for frac entering eps = 1 - frac (through pref and ds), the second for the numerator of eta.  Under POL the exact
first-order difference between cth = k_i . k_j / kmag^2 and 1 - |q|^2 / (2 kmag^2) -- (|k_i|^2 + |k_j|^2 - 2 kmag^2) / (2 kmag^2),
which is the model's ambiguity between the two kernels' statements, not a rounding error -- enters as |G_ij I_j| |cth delta / 2| / f
in units of 2^-53 (it is itself of that size, so it is scaled by 2^53 to stand beside the other terms).  A clamped pair has
|G_clamped I_j| (1 + frac / eps) alone: lim / sqrt(Ii Ij) does not depend on eta, and the clamp is continuous at w = lim.  One
exception, found when c_ref was first measured: the clamped gain is sign(G) lim / sqrt(Ii Ij), and where eta sits within rounding
of zero while |G| is still beyond the limit (extreme intensities, eta = 0 through a cancelling numerator) one rounding of the
numerator flips its sign -- the IEEE statements are 9e9 units from the model there.  The clamp is 1-Lipschitz in G, so the
unclamped pair's eta term bounds the clamped pair's error; it is kept for the clamped pairs that are not FIRM: those whose swing
w does not stay above lim when G moves by FIRM = 2^10 units of its own eta term (`soft` counts them: a handful per set).
Errors are counted in units u = |K - K_ref| / (2^-53 S_i)."""
import numpy as np

from helpers import bandwidth_cases as BC

KC = 29979245800.0
SHAPE = (4, 3, 148)
GRID = (6, 5, 150)
NODES = SHAPE[0] * SHAPE[1] * SHAPE[2]
UNIT = 2.0 ** -53
ANGLES = (1e-9, 1e-6, 1e-3, 0.3, 1.2, np.pi / 2, 2.5, np.pi - 1e-6, np.pi)
# ... and the peak of P at the default iaw = 0.2, where P' = 0: the eta term of S vanishes there and S is |K| (1 + frac / eps)
# alone, the tightest scale of the sweep -- added so that a pair function without its reciprocal's Newton step or its quotient's
# correction (an error of 2^-46 of G = 128 units of G) is caught beyond 4 x the bound (tests/test_pair_accuracy_host.py)
PEAK = float(np.sqrt(((2 - 0.04) + np.sqrt((2 - 0.04) ** 2 + 12)) / 6))
ETAS = (0.0,) + tuple(s * v for v in (1e-8, 1e-3, 0.5, PEAK, 1 - 1e-6, 1 - 1e-12, 1.0, 1 + 1e-9, 2.0, 30.0, 1e3, 1e6) for s in (1, -1))
FRACS = (1e-3, 0.1, 0.25, 0.7, 0.99, 1 - 1e-6)
CONSTRUCTIONS = ("along", "perpendicular", "beat")
KINDS = ("crossed", "ulp", "supercritical", "absent", "parallel")
NCROSSED, NULP, NZERO = 1600, 32, 48                      # crossed cases, ulp-apart pairs, and each of the three zero blocks
assert NCROSSED + NULP + 3 * NZERO == NODES and 3 * NZERO <= 0.15 * NODES and len(ANGLES) == 9 and len(ETAS) == 25
DW = float(round(4.6e12 / 2.0 ** 24) * 2.0 ** 24)        # the beat frequency of every designed pair, rad/s (detuning_cases' scale)
SPECTRUM = "three"                                        # bandwidth_cases' 3-line spectrum
# the options sets: (DETUNE, POL, BAND, SAT); the limit of a SAT set is the median pair amplitude of the set it clamps
OPTIONS = {"plain": (False, False, False, False), "detune": (True, False, False, False), "pol": (False, True, False, False),
           "all": (True, True, True, False), "sat": (False, False, False, True), "sat_all": (True, True, True, True)}
ORDER = tuple(OPTIONS)
CLAMPS = {"sat": "plain", "sat_all": "all"}
WORLDS = ("A", "B")
NBEAMS = {"A": 2, "B": 60}
# c_ref: the worst error of the IEEE ordered statements against the model, units of 2^-53 S (tests/test_pair_accuracy_host.py
# measures it on the CPU and asserts it is no larger); the device bound of a set is 4 x ceil(c_ref): x 2 for the pair-once form's
# roughly double count of roundings (about 20 fused operations in its three chains against about 12 ordered statements, and K_i a
# sum of up to three such terms in another grouping), x 2 of headroom.  Never taken from a kernel.
C_REF = {"plain": 3.721, "detune": 4.260, "pol": 3.861, "all": 2.639, "sat": 4.675, "sat_all": 4.443}
FIRM = 2.0 ** 10                                          # a clamped pair is firm if it stays clamped under this many units
PERIODS = (6, 11, 20)                                     # world B: distinct beam triples per z period of a row, by row class


def bound(option):
    """The device bound of an options set, in units of 2^-53 S."""
    return 4 * int(np.ceil(C_REF[option]))


def triple(row, hk):
    """World B: the triple m (beams 3 m, 3 m + 1, 3 m + 2) of haloed cell hk of interior row `row` = 0 .. 11.  16 cells of a row
    of class row % 3 hold 18, 33 and 48 beams."""
    period = PERIODS[row % 3]
    return ((hk + 5 * row) % period + 3 * row) % 20


def shifts(world):
    """Per-beam frequency shifts, multiples of 2^24 rad/s so that every difference is exact; beams 0 and 1 of world A and
    beams 3 m, 3 m + 1 of world B are DW apart."""
    if world == "A":
        return np.array([0.0, DW])
    out = np.zeros(60)
    for m in range(20):
        base = (m - 10) * 2.0 ** 36
        out[3 * m:3 * m + 3] = base, base + DW, base - 3.0 * 2.0 ** 38
    return out


def _unit(v):
    return v / np.sqrt(v @ v)


def _kvec(kmag, a):
    dn = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    return kmag * (a / dn)


def _f32(x):
    """A double that float32 holds exactly (energies, cs, gain_const: stored as float32 in the fixture)."""
    return float(np.float32(x))


def build_inputs(consts):
    """The inputs of both worlds from consts = dict(ncrit, omega, dt, iaw): ne3d [4, 3, 148], flow [3, ...], state [2, ...],
    E [3, ...] the energies of A's two beams and B's third, k [3, 3, ...] their k vectors (beam, component), and the case of
    every node: angle, eta, construction, frac, kind (indices into the tuples above, -1 where the axis does not apply)."""
    ncrit, omega = consts["ncrit"], consts["omega"]
    rng = np.random.default_rng(20261021)
    k0 = omega / KC
    node_of = rng.permutation(NODES)
    ne, cs, gc = np.zeros(NODES), np.zeros(NODES), np.zeros(NODES)
    u, E, k = np.zeros((3, NODES)), np.zeros((3, NODES)), np.zeros((3, 3, NODES))
    meta = {name: np.full(NODES, -1, dtype=np.int16) for name in ("angle", "eta", "construction", "frac", "kind")}
    for c in range(NODES):
        n = node_of[c]
        ai, ei, ci = c % 9, (c // 9) % 25, (c // 225) % 3
        fi = (ai + ei + ci + 3 * (c // 675)) % 6
        kind = 0 if c < NCROSSED else (1 if c < NCROSSED + NULP else 2 + (c - NCROSSED - NULP) // NZERO)
        sub = (c - NCROSSED - NULP) % NZERO                                    # the case's number inside a zero block
        ne[n] = FRACS[fi] * ncrit
        if kind == 2:
            ne[n] = (ncrit, np.nextafter(ncrit, np.inf), 1.5 * ncrit)[sub % 3]
        frac = ne[n] / ncrit
        eps = 1.0 - frac
        rt = np.sqrt(eps) if eps > 0 else 0.0
        kmag = k0 * rt if eps > 0 else k0                                      # super-critical: any k, the kernels must not use it
        cs[n] = _f32(10.0 ** rng.uniform(6.5, 7.8))
        gc[n] = _f32(7e-13 * 10.0 ** rng.uniform(-1.0, 1.0))
        E[:, n] = [_f32(10.0 ** e) for e in rng.uniform(8.0, 14.0, 3)]
        a = _unit(rng.normal(size=3))
        p = _unit(np.cross(a, rng.normal(size=3)))
        theta = ANGLES[ai]
        ka, kb = _kvec(kmag, a), _kvec(kmag, a * np.cos(theta) + p * np.sin(theta))
        if kind == 1:                                                          # one ulp apart in one component
            kb = ka.copy()
            kb[c % 3] = np.nextafter(ka[c % 3], np.inf if c & 4 else -np.inf)
            ci = 2 * (c & 1)                                                   # along or beat
        if kind == 4:
            kb = ka.copy()
        p2 = _unit(np.cross(a, rng.normal(size=3)))
        third = ANGLES[(ai + 4) % 9]
        k[0, :, n], k[1, :, n], k[2, :, n] = ka, kb, _kvec(kmag, a * np.cos(third) + p2 * np.sin(third))
        # the flow that puts eta of the pair (a, b) where the case wants it
        eta = ETAS[ei]
        q = kb - ka
        q2 = q @ q
        rand = rng.normal(size=3)
        if q2 == 0.0:
            u[:, n] = 1e7 * rand
        else:
            D = np.sqrt(q2) * cs[n] + 1e-10
            if ci == 0:
                u[:, n] = q * (-eta * D / q2)
            elif ci == 1:
                perp = _unit(rand - q * ((rand @ q) / q2))
                u[:, n] = 4e7 * perp + q * (-eta * D / q2)
            else:
                free = 1e7 * rand
                u[:, n] = free + q * ((DW - eta * D - q @ free) / q2)
        if kind == 3:                                                          # a or b absent: untouched, or touched without energy
            E[(sub >> 1) & 1, n] = 0.0 if sub & 1 else -E[(sub >> 1) & 1, n]
        meta["kind"][n] = kind
        meta["frac"][n] = fi if kind != 2 else -1
        if kind in (0, 1):
            meta["eta"][n], meta["construction"][n] = ei, ci
        if kind == 0:
            meta["angle"][n] = ai
    shaped = lambda x: np.ascontiguousarray(x.reshape(x.shape[:-1] + SHAPE))   # noqa: E731
    out = dict(ne3d=shaped(ne), flow=shaped(u), state=shaped(np.stack([cs, gc])), E=shaped(E), k=shaped(k))
    out.update({name: shaped(v) for name, v in meta.items()})
    return out


def slots():
    """World B: the triple of every node, [4, 3, 148]."""
    out = np.zeros(SHAPE, dtype=np.int8)
    for i in range(SHAPE[0]):
        for j in range(SHAPE[1]):
            out[i, j] = [triple(i * SHAPE[1] + j, kk + 1) for kk in range(SHAPE[2])]
    return out


def fields(inp, world):
    """The field arrays [4, nbeams, 6, 5, 150] of a world as the frozen kernels read them: (E, kx, ky, kz), zeros in the halo."""
    out = np.zeros((4, NBEAMS[world]) + GRID)
    inner = (slice(1, -1),) * 3
    if world == "A":
        for b in range(2):
            out[0, b][inner] = inp["E"][b]
            for comp in range(3):
                out[1 + comp, b][inner] = inp["k"][b, comp]
        return out
    m = slots()
    for t in range(20):
        here = m == t
        for b in range(3):
            out[0, 3 * t + b][inner] = np.where(here, inp["E"][b], 0.0)
            for comp in range(3):
                out[1 + comp, 3 * t + b][inner] = np.where(here, inp["k"][b, comp], 0.0)
    return out


def run_classes(raw):
    """crowded_world's count: the 16-cell windows beyond the first 64 cells of a row that hold <= 20, 21 - 40 and > 40 present
    beams."""
    present = raw[0] > 0
    windows = np.stack([present[..., z0:z0 + 16].any(-1).sum(0) for z0 in range(64, GRID[2], 16)])
    return [int(((windows > 0) & (windows <= 20)).sum()), int(((windows > 20) & (windows <= 40)).sum()), int((windows > 40).sum())]


# ---- the model ------------------------------------------------------------------------------------------------------------
def _resonance(eta, iaw2):
    """P(eta) and P'(eta)."""
    e2 = eta * eta
    t = e2 - 1
    den = t * t + iaw2 * e2
    return iaw2 * eta / den, iaw2 * (den - eta * (4 * eta * t + 2 * iaw2 * eta)) / (den * den)


def _pairs(mp, inp, consts, lines):
    """Stage 1: per node the cell's factors and, per world, the evaluated pairs with the unclamped gain, its eta sensitivity
    and its POL ambiguity for the four unclamped sets."""
    f = mp.mpf
    ncrit, omega, dt, iaw = (f(consts[key]) for key in ("ncrit", "omega", "dt", "iaw"))
    iaw2, k0, c = iaw * iaw, omega / f(KC), f(KC)
    offs = [f(float(o)) for o in lines[0]]
    wsum = sum(f(float(w)) for w in lines[1])
    wts = [f(float(w)) / wsum for w in lines[1]]
    band = [(offs[b] - offs[a], wts[a] * wts[b]) for a in range(len(offs)) for b in range(len(offs))]
    sh = {w: shifts(w) for w in WORLDS}
    m3 = slots().reshape(-1)
    flat = {key: inp[key].reshape(inp[key].shape[:-3] + (NODES,)) for key in ("ne3d", "flow", "state", "E", "k")}
    cells = []
    for n in range(NODES):
        frac = f(float(flat["ne3d"][n])) / ncrit
        eps = 1 - frac
        cell = dict(sub=eps > 0, pairs={w: [] for w in WORLDS})
        cells.append(cell)
        if not cell["sub"]:
            continue
        rt = mp.sqrt(eps)
        ds, kmag = c * rt * dt, k0 * rt
        cs, gc = f(float(flat["state"][0, n])), f(float(flat["state"][1, n]))
        pref, kap = gc * frac * (1 / iaw) / rt, (k0 / 2) * frac / rt
        u = [f(float(flat["flow"][comp, n])) for comp in range(3)]
        kv = [[f(float(flat["k"][b, comp, n])) for comp in range(3)] for b in range(3)]
        E = [float(flat["E"][b, n]) for b in range(3)]
        inten = [f(E[b]) / ds if E[b] > 0 and any(x != 0 for x in kv[b]) else f(0) for b in range(3)]
        cell.update(ds=ds, kap=kap, cond=1 + frac / eps, I=inten)
        done = {}
        for w in WORLDS:
            beams = (0, 1) if w == "A" else (0, 1, 2)
            number = (0, 1) if w == "A" else tuple(3 * int(m3[n]) + b for b in range(3))
            for i in beams:
                for j in beams[i + 1:]:
                    if not (inten[i] > 0 and inten[j] > 0):
                        continue
                    q = [kv[j][comp] - kv[i][comp] for comp in range(3)]
                    q2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2]
                    if q2 == 0:
                        continue
                    dw = f(float(sh[w][number[j]])) - f(float(sh[w][number[i]]))
                    key = (i, j, dw)
                    if key not in done:
                        D = mp.sqrt(q2) * cs + f(1e-10)
                        prods = [q[comp] * u[comp] for comp in range(3)]
                        N0, T0 = -(prods[0] + prods[1] + prods[2]), abs(prods[0]) + abs(prods[1]) + abs(prods[2])
                        P, dP = _resonance(N0 / D, iaw2)
                        plain = (pref * P, abs(pref * dP) * T0 / D)
                        P, dP = _resonance((N0 + dw) / D, iaw2)
                        detune = (pref * P, abs(pref * dP) * (T0 + abs(dw)) / D)
                        sP, sS = f(0), f(0)
                        for d, pp in band:
                            P, dP = _resonance((N0 + dw + d) / D, iaw2)
                            sP += pp * P
                            sS += pp * abs(dP) * (T0 + abs(dw) + abs(d))
                        banded = (pref * sP, abs(pref) * sS / D)
                        kk = kmag * kmag
                        cth = (kv[i][0] * kv[j][0] + kv[i][1] * kv[j][1] + kv[i][2] * kv[j][2]) / kk
                        fac = (1 + cth * cth) / 4
                        delta = (sum(x * x for x in kv[i]) + sum(x * x for x in kv[j]) - 2 * kk) / (2 * kk)
                        amb = abs(cth * delta / 2) / fac * f(2) ** 53
                        done[key] = {"plain": plain + (f(0),), "detune": detune + (f(0),),
                                     "pol": (plain[0] * fac, plain[1] * fac, amb), "all": (banded[0] * fac, banded[1] * fac, amb)}
                    cell["pairs"][w].append((i, j, done[key]))
    return cells


def model(inp, consts):
    """The 200-bit model of both worlds.  Returns dict(sat {world: {set: dn_max}} the limits of the SAT sets as doubles: the
    median pair amplitude of the set each clamps; share {world: {set: clamped share of the present pairs}}; soft {world: {set:
    clamped pairs that are not firm}}; K {world: {set: mpf [beam][node]}}, S likewise; live {world: bool [beam, node]: some pair
    of the entry is evaluated}; T {set: dict(T, G, scaled, cells)} the exchange of world A's pair for plain and sat: the sum of
    x = ds g I_0 I_1 and of |x|, the sum of ds I_0 S_0, and the number of cells with a term)."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.prec = 200
    f = mp.mpf
    cells = _pairs(mp, inp, consts, BC.lines(SPECTRUM))
    nloc = {"A": 2, "B": 3}
    sat = {w: {} for w in WORLDS}
    for w in WORLDS:
        for name, base in CLAMPS.items():
            amps = sorted(abs(rec[base][0]) * mp.sqrt(c["I"][i] * c["I"][j]) / c["kap"]
                          for c in cells if c["sub"] for i, j, rec in c["pairs"][w])
            sat[w][name] = float(amps[len(amps) // 2])
    K = {w: {o: [[f(0)] * NODES for _ in range(nloc[w])] for o in ORDER} for w in WORLDS}
    S = {w: {o: [[f(0)] * NODES for _ in range(nloc[w])] for o in ORDER} for w in WORLDS}
    live = {w: np.zeros((nloc[w], NODES), dtype=bool) for w in WORLDS}
    share = {w: {o: [0, 0] for o in CLAMPS} for w in WORLDS}
    soft = {w: {o: 0 for o in CLAMPS} for w in WORLDS}
    T = {o: dict(T=f(0), G=f(0), scaled=f(0), cells=0) for o in ("plain", "sat")}
    for n, c in enumerate(cells):
        if not c["sub"]:
            continue
        for w in WORLDS:
            for i, j, rec in c["pairs"][w]:
                Ii, Ij = c["I"][i], c["I"][j]
                live[w][i, n] = live[w][j, n] = True
                for o in ORDER:
                    g, sens, amb = rec[CLAMPS.get(o, o)]
                    firm = False
                    if o in CLAMPS:
                        lim, root = f(sat[w][o]) * c["kap"], mp.sqrt(Ii * Ij)
                        swing = abs(g) * root
                        clamped = swing > lim
                        firm = clamped and swing - FIRM * UNIT * sens * root >= lim
                        share[w][o][0] += int(clamped)
                        share[w][o][1] += 1
                        soft[w][o] += int(clamped and not firm)
                        if clamped:
                            g = g * (lim / swing)
                    K[w][o][i][n] += g * Ij
                    K[w][o][j][n] -= g * Ii
                    for a, Ib in ((i, Ij), (j, Ii)):
                        S[w][o][a][n] += abs(g * Ib) * c["cond"] + (0 if firm else Ib * sens + abs(g * Ib) * amb)
                    if w == "A" and o in T:
                        x = c["ds"] * g * Ii * Ij
                        T[o]["T"] += x
                        T[o]["G"] += abs(x)
                        T[o]["cells"] += 1
        for o in T:
            T[o]["scaled"] += c["ds"] * c["I"][0] * S["A"][o][0][n]
    share = {w: {o: v[0] / max(v[1], 1) for o, v in d.items()} for w, d in share.items()}
    return dict(sat=sat, share=share, soft=soft, K=K, S=S, live=live, T=T, mp=mp)


def split(mp, x):
    """An mpf as a double-double: (hi, lo in units of 2^-53 |hi|)."""
    hi = float(x)
    if hi == 0.0:
        return 0.0, 0.0
    return hi, float((x - mp.mpf(hi)) / (mp.mpf(UNIT) * abs(mp.mpf(hi))))


def pack(inp, consts, ref):
    """The fixture's arrays: the inputs (energies and the state table as float32, which holds them exactly), the constants, and
    per world and options set K_ref as hi (float64) and lo (float16, in units of 2^-53 |hi|: the pair is good to 2^-64 of K)
    and log2 S as float32 (-inf for S = 0): S spans 85 decades, and is read back good to 1e-5 of itself."""
    mp = ref["mp"]
    out = dict(ne3d=inp["ne3d"], flow=inp["flow"], k=inp["k"], state=inp["state"].astype(np.float32), E=inp["E"].astype(np.float32),
               slot=slots(), line_offsets=BC.lines(SPECTRUM)[0], line_weights=BC.lines(SPECTRUM)[1],
               consts=np.array([consts[key] for key in ("ncrit", "omega", "dt", "iaw")]))
    assert np.array_equal(out["state"].astype(np.float64), inp["state"]) and np.array_equal(out["E"].astype(np.float64), inp["E"])
    for name in ("angle", "eta", "construction", "frac", "kind"):
        out[name] = inp[name].astype(np.int8)
    for w in WORLDS:
        out["shift_" + w] = shifts(w)
        out["sat_" + w] = np.array([ref["sat"][w][o] for o in CLAMPS])
        out["share_" + w] = np.array([ref["share"][w][o] for o in CLAMPS])
        out["soft_" + w] = np.array([ref["soft"][w][o] for o in CLAMPS])
        out["live_" + w] = ref["live"][w].reshape((-1,) + SHAPE)
        nloc = len(ref["K"][w][ORDER[0]])
        hi, lo, s = (np.zeros((len(ORDER), nloc, NODES)) for _ in range(3))
        for oi, o in enumerate(ORDER):
            for b in range(nloc):
                for n in range(NODES):
                    hi[oi, b, n], lo[oi, b, n] = split(mp, ref["K"][w][o][b][n])
                    sv = ref["S"][w][o][b][n]
                    s[oi, b, n] = float(mp.log(sv, 2)) if sv > 0 else -np.inf
        s32 = s.astype(np.float32)
        shape = (len(ORDER), nloc) + SHAPE
        out["hi_" + w], out["lo_" + w], out["S_" + w] = hi.reshape(shape), lo.astype(np.float16).reshape(shape), s32.reshape(shape)
    for o, t in ref["T"].items():
        out["T_" + o] = np.array([float(t["T"]), float(t["G"]), float(t["scaled"]), float(t["cells"])])
    return out


# ---- reading the fixture --------------------------------------------------------------------------------------------------
def constants(fx):
    return dict(zip(("ncrit", "omega", "dt", "iaw"), (float(v) for v in fx["consts"])))


def inputs_of(fx):
    """build_inputs' dict from the fixture's arrays."""
    out = {key: np.asarray(fx[key], dtype=np.float64) for key in ("ne3d", "flow", "k", "state", "E")}
    out.update({name: np.asarray(fx[name]).astype(np.int16) for name in ("angle", "eta", "construction", "frac", "kind")})
    return out


def haloed(world, per_node):
    """Per-node arrays [nloc, 4, 3, 148] of a world on its haloed beam grids [nbeams, 6, 5, 150], zeros elsewhere."""
    out = np.zeros((NBEAMS[world],) + GRID, dtype=per_node.dtype)
    inner = (slice(1, -1),) * 3
    if world == "A":
        for b in range(2):
            out[b][inner] = per_node[b]
        return out
    m = slots()
    for t in range(20):
        for b in range(3):
            out[3 * t + b][inner] = np.where(m == t, per_node[b], 0)
    return out


def reference(fx, world, option):
    """(hi, lo, S, live) of a world and options set on the haloed beam grids: K_ref = hi + lo as doubles, S as float64."""
    oi = ORDER.index(option)
    hi = np.asarray(fx["hi_" + world][oi], dtype=np.float64)
    lo = np.asarray(fx["lo_" + world][oi], dtype=np.float64) * (UNIT * np.abs(hi))
    s = np.exp2(np.asarray(fx["S_" + world][oi], dtype=np.float64))
    return haloed(world, hi), haloed(world, lo), haloed(world, s), haloed(world, np.asarray(fx["live_" + world]))


def errors(K, hi, lo):
    """|K - (hi + lo)| in double: K - hi is exact where K is within a factor 2 of hi, and lo is below half an ulp of hi."""
    return np.abs((K - hi) - lo)


def describe(fx, cell):
    """The case of haloed cell (hi, hj, hk) in words."""
    i, j, kk = (int(x) - 1 for x in cell)
    pick = lambda name, values: values[int(fx[name][i, j, kk])] if int(fx[name][i, j, kk]) >= 0 else None   # noqa: E731
    return "node (%d, %d, %d): %s, angle %s, eta %s, %s, frac %s" % (i, j, kk, pick("kind", KINDS), pick("angle", ANGLES),
                                                                     pick("eta", ETAS), pick("construction", CONSTRUCTIONS), pick("frac", FRACS))
