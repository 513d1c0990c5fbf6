"""What tests/test_mixing_host.py and tests/test_gpu_mixing.py share: the numpy restatement of the two
mixing passes, the arrays they run on, a linear toy engine for cbet_fixed_point, and the oracle engine of
tests/test_cbet_model.py with the host mixing mixed in."""
import math

import numpy as np
import torch

from cbet_raytracing_3d_amd.cbet_loop import HostMixing

SIZES = [1, 2, 63, 64, 65, 255, 4097]        # a single element, around a wavefront, odd, two spans and one element


def arrays(n, count, seed):
    """y, x and `count` held arrays of n doubles with mixed signs and magnitudes (so that sums cancel)."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n) for _ in range(count + 2)]


def residual_numpy(y, x, f_held):
    """(f, row, scale): f = y - x elementwise, row[j] = fsum(f * f_held[j]), row[h] = fsum(f * f), and per entry the
    sum of |a * b| its bound is stated in."""
    f = y - x
    others = list(f_held) + [f]
    row = np.array([math.fsum((f * g).tolist()) for g in others])
    scale = np.array([math.fsum(np.abs(f * g).tolist()) for g in others])
    return f, row, scale


def apply_numpy(y_held, alpha):
    """acc = alpha_0 y_0; acc = acc + alpha_j y_j, oldest first: one IEEE operation per operator (numpy fuses nothing)."""
    acc = alpha[0] * y_held[0]
    for a, y in zip(alpha[1:], y_held[1:]):
        acc = acc + a * y
    return acc


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


class ToyEngine(HostMixing):
    """y = x + relax (d o x + b - x) on n numbers: a linear map whose Jacobian has as many distinct eigenvalues as d has
    distinct values.  switch_at: from that update on (counted from 0) the map uses b2 instead of b.  Records every x it
    was given, every y it made and every residual norm."""

    def __init__(self, d, b, relax, switch_at=None, b2=None):
        self.d, self.b, self.relax, self.switch_at, self.b2 = d, b, relax, switch_at, b2

    def begin(self):
        self.gain = np.zeros_like(self.b)
        self.seen, self.made, self.res = [], [], []

    def field_passes(self, use_gain, si, sc, full=True):
        return torch.zeros(4, 1, dtype=torch.float64)

    def update_gain(self, fields, frozen=False):
        x = self.gain
        b = self.b2 if (self.switch_at is not None and len(self.seen) >= self.switch_at) else self.b
        y = x + self.relax * (self.d * x + b - x)
        self.seen.append(x.copy())
        self.made.append(y.copy())
        self.res.append(float(np.linalg.norm(y - x)))
        self.gain = y
        return torch.tensor([np.abs(y - x).sum(), np.abs(y).sum()], dtype=torch.float64)

    def deposit(self, si, sc):
        return torch.zeros(1, dtype=torch.float64)


def mixed_oracle_engine(O, api, cfg, g, bn, ne3d, kap, nbeams, nthreads=2):
    """tests/test_cbet_model.py's oracle engine with the host mixing mixed in (and `nthreads` oracle threads per pass)."""
    from test_cbet_model import _OracleEngine

    class Engine(HostMixing, _OracleEngine):
        def field_passes(self, use_gain, si, sc, full=True):
            qs = (1, 2, 3, 4) if full else (1,)
            F = [O.trace_cbet(self.cfg, self.g, self.bn, self.ne3d, self.kap, gain=self.gain if use_gain else None,
                              quantity=q, per_beam=True, nthreads=nthreads, items=self._items(si, sc))[0] for q in qs]
            if full:
                self.fields = torch.from_numpy(np.stack(F))
            else:
                self.fields[0] = torch.from_numpy(F[0])
            return self.fields

        def update_gain(self, fields, frozen=False):
            self.gain, ch = O.gain_field(self.cfg, self.g, fields.numpy(), self.ne3d, relax=self.relax, gain=self.gain, nthreads=nthreads)
            return torch.tensor(ch, dtype=torch.float64)

        def deposit(self, si, sc):
            e, steps, bg = O.trace_cbet(self.cfg, self.g, self.bn, self.ne3d, self.kap, gain=self.gain, nthreads=nthreads,
                                        items=self._items(si, sc))
            self.edep += e
            self.steps = steps
            return torch.from_numpy(bg)

    eng = Engine(O, api, cfg, g, bn, ne3d, kap, nbeams)
    eng.relax = 1.0
    return eng
