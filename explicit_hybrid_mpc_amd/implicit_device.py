"""
The implicit law in closed loop with the whole loop on the device (``ehm_implicit_rollout``,
csrc/ehm_implicit.hip): what ``simulate.rollout_implicit(..., on_device=True)`` runs.

Per step a fixed sequence of launches on the oracle's stream -- measure, phase one for the
n * n_delta (trajectory, commutation) pairs, compaction of the feasible ones, their point solve,
the minimum with the tie rule of ``ehm_solve_pt_batch``, the plant step with the noise draws -- with
state, last input, status and accumulators resident on the device; records are written there and
copied once at the end.  The two solves are the launches ``solve_pt`` makes, so a step returns
``solve_pt``'s input and commutation bit for bit -- except where a solve stalls (non-zero status):
the host path repeats a stalled LP of either solve on the generation-1 kernels, the device loop
cannot.  A stalled phase-one solve keeps the tau it reached (the verdict may differ from the
host's); a feasible pair whose point solve stalls is left out of the minimum.  Both are counted
(``n_stalled_pairs``, of which ``n_stalled_phase_one``) and the trajectory is flagged
(``stalled``).  Flagged trajectories may differ from the host loop's.

The step's arithmetic is fixed (sums in column order from 0.0, no FMA; ``simulate._dot_rows``):
x+ = ((A x) + (B (u + e))) + w, then + (E d); tests/implicit_cpu.py is the numpy mirror.
"""

import ctypes

import numpy as np

from . import _capi
from ._capi import f64, ptr

MAX_P, MAX_NU = 8, 4
# device memory one call may take for its pairs and records (the cap of the export staging)
CHUNK_BYTES = 768 << 20


_check = _capi.checker('ehm_implicit_last_error')


def check_args(oracle, plant):
    """The refusals of the device loop, before any use of the device."""
    can = getattr(oracle, 'canonical', None)
    if can is None or getattr(oracle, 'gpu', None) is None:
        raise ValueError('on_device needs an oracle whose commutations are enumerated '
                         '(oracle.Oracle), not %s' % type(oracle).__name__)
    if can.n_u > MAX_NU or can.p > MAX_P:
        raise ValueError('on_device takes n_u <= %d and p <= %d (n_u %d, p %d)' % (
            MAX_NU, MAX_P, can.n_u, can.p))
    if plant.n_x != can.p or plant.n_u != can.n_u:
        raise ValueError('plant (n_x %d, n_u %d) does not fit the law (p %d, n_u %d)' % (
            plant.n_x, plant.n_u, can.p, can.n_u))


def chunk_size(n_delta, p, n_u, n_d, T, record, noisy, budget=CHUNK_BYTES, given_d=False,
               given_v=False):
    """Trajectories per call such that pairs, state, records and the device copies of a caller's
    d and v stay within ``budget`` bytes."""
    per = n_delta * (48 + 8 * n_u) + 8 * (3 * p + 3 * n_u + 8)
    per += 8 * T * ((n_d if given_d else 0) + (p if given_v else 0))
    if record:
        per += 8 * (T + 1) * p + T * (8 * n_u + 8)
        if noisy:
            per += 8 * T * (p + n_u + n_d)
    return max(1, int(budget // per))


class ImplicitDevice:
    """The device loop's handle for one oracle: holds the plant and the noise model."""

    def __init__(self, oracle):
        self._lib = _capi.load()
        self._gpu = oracle.gpu            # the solver handle must outlive this one
        self._handle = ctypes.c_void_p()
        self.can = oracle.canonical
        self.mode_of = np.ascontiguousarray(
            [oracle.mpc.step0_mode(dl) for dl in self.can.deltas], dtype=np.int32)
        _check(self._lib.ehm_implicit_create(self._gpu._handle, ctypes.byref(self._handle)))
        self._noise_packed = None

    @property
    def open(self):
        """Both this handle and the solver handle it borrows are alive."""
        return bool(self._handle) and bool(self._gpu._handle)

    def close(self):
        if getattr(self, '_handle', None):
            self._lib.ehm_implicit_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_plant(self, plant):
        opt = lambda a: ptr(a) if a.size else None
        A, B, w, Gx, gx, Q, R = (f64(a) for a in (plant.A, plant.B, plant.w, plant.Gx, plant.gx,
                                                  plant.Q, plant.R))
        if plant.guarded:
            gm, row0, ga, gb, gc, gt, st = plant.guard_arrays()
            ga, gb, gc, gt = f64(ga), f64(gb), f64(gc), f64(gt)
            fn = self._lib.ehm_implicit_set_plant_guarded
            own = (plant.substeps, len(gm), opt(gm), ptr(row0), opt(ga), opt(gb), opt(gc), opt(gt),
                   opt(st), plant.default_mode)
        else:
            rows, H, h = plant.region_arrays()
            E, H, h = f64(plant.E), f64(H), f64(h)
            fn = self._lib.ehm_implicit_set_plant
            own = (plant.n_d, opt(E), ptr(rows), opt(H), opt(h))
        _check(fn(self._handle, plant.n_modes, ptr(A), ptr(B), ptr(w), *own, plant.gx.size, opt(Gx),
                  opt(gx), ptr(self.mode_of), 0 if plant.cost == 'inf' else 1, ptr(Q), ptr(R)))

    def set_noise(self, model, plant):
        desc, data = model.pack()
        held = self._noise_packed
        if held is not None and held[2] == plant.n_d and np.array_equal(held[0], desc) \
                and np.array_equal(held[1], data):
            return
        self._noise_packed = None
        _check(self._lib.ehm_implicit_set_noise(self._handle, desc.shape[0], ptr(desc),
                                                ptr(data) if data.size else None, data.size,
                                                plant.n_d))
        self._noise_packed = (desc, data, plant.n_d)

    def run(self, plant, X0, T, d, v, record, tol_exit, noise, seed, traj0):
        """One call of ehm_implicit_rollout: a dict of its outputs."""
        n, p = X0.shape
        n_u, n_d = self.can.n_u, plant.n_d
        rec = lambda shape, dtype=np.float64: np.empty(shape, dtype) if record else None
        o = dict(x=rec((T + 1, n, p)), u=rec((T, n, n_u)), commutation=rec((T, n), np.int32),
                 mode=rec((T, n), np.int32), v=None, e=None, w=None)
        if noise is not None:
            o.update(v=rec((T, n, p)), e=rec((T, n, n_u)), w=rec((T, n, n_d)))
        o.update(x_final=np.empty((n, p)), steps=np.empty(n, np.int32),
                 status=np.empty(n, np.int32), cost=np.empty(n), u_norm_sum=np.empty(n),
                 max_violation=np.empty(n), stalled=np.empty(n, np.int32))
        counts = np.zeros(5, dtype=np.int64)
        secs = ctypes.c_double(0.)
        _check(self._lib.ehm_implicit_rollout(
            self._handle, n, T, ptr(X0), ptr(d), ptr(v), 0 if noise is None else 1, int(seed),
            int(traj0), float(tol_exit), ptr(o['x']), ptr(o['u']), ptr(o['commutation']),
            ptr(o['mode']), ptr(o['v']), ptr(o['e']), ptr(o['w']), ptr(o['x_final']),
            ptr(o['steps']), ptr(o['status']), ptr(o['cost']), ptr(o['u_norm_sum']),
            ptr(o['max_violation']), ptr(o['stalled']), ptr(counts), ctypes.addressof(secs)))
        o['counts'] = counts
        o['seconds'] = secs.value
        return o


def rollout(oracle, plant, X0, T, d=None, v=None, record=True, tol_exit=1e-9, noise=None, seed=0,
            traj0=0, chunk=None):
    """
    ``simulate.rollout_implicit`` on the device (arguments already checked by it).  The batch is
    split into chunks that fit the device memory budget (``chunk`` trajectories; default
    ``chunk_size``); the draws do not depend on the split (trajectory q has id traj0 + q).
    Returns a ``simulate.ClosedLoop`` with, beyond the host loop's fields, ``stalled`` bool [n],
    ``n_stalled_pairs`` (both solves; ``n_stalled_phase_one`` of them in phase one), ``lp_solves``
    (phase one, point) and ``launches``; ``seconds`` is the
    device time between the first and the last launch, summed over the chunks.
    """
    from . import simulate
    n, p = X0.shape
    T = int(T)
    dev = getattr(oracle, '_implicit_device', None)
    if dev is None or not dev.open or dev._gpu is not oracle.gpu:
        if not oracle.gpu._handle:
            raise ValueError('the oracle is closed')
        dev = oracle._implicit_device = ImplicitDevice(oracle)
    dev.set_plant(plant)          # a few KB: every call, so a plant changed in place is seen
    if noise is not None:
        dev.set_noise(noise, plant)
    if chunk is None:
        chunk = chunk_size(dev.can.n_delta, p, dev.can.n_u, plant.n_d, T, record,
                           noise is not None, given_d=d is not None, given_v=v is not None)
    cut = lambda a, lo, hi: None if a is None else np.ascontiguousarray(a[:, lo:hi])
    parts = [dev.run(plant, np.ascontiguousarray(X0[lo:lo + chunk]), T, cut(d, lo, lo + chunk),
                     cut(v, lo, lo + chunk), record, tol_exit, noise, seed, int(traj0) + lo)
             for lo in range(0, n, chunk)]
    if not parts:
        parts = [dev.run(plant, X0, T, d, v, record, tol_exit, noise, seed, traj0)]
    cat = lambda k, axis: None if parts[0][k] is None else (
        parts[0][k] if len(parts) == 1 else np.concatenate([q[k] for q in parts], axis=axis))
    counts = sum(q['counts'] for q in parts)
    out = simulate.ClosedLoop(
        x_final=cat('x_final', 0), steps=cat('steps', 0), status=cat('status', 0),
        cost=cat('cost', 0), u_norm_sum=cat('u_norm_sum', 0), max_violation=cat('max_violation', 0),
        seconds=float(sum(q['seconds'] for q in parts)), stalled=cat('stalled', 0).astype(bool),
        n_stalled_pairs=int(counts[0]), n_stalled_phase_one=int(counts[4]), lp_solves=(int(counts[1]), int(counts[2])),
        launches=int(counts[3]))
    if record:
        out.x, out.u, out.commutation = cat('x', 1), cat('u', 1), cat('commutation', 1)
        out.mode = None if plant.guarded else cat('mode', 1)
        if noise is not None:
            out.v, out.e, out.w = cat('v', 1), cat('e', 1), cat('w', 1)
    return out
