"""
The compiled law's closed loop on the host (no GPU): the numpy mirror of k_compiled_rollout
(tests/compiled_rollout_cpu) on host-compiled arrays against exact arithmetic and against the exact
host rollout of the source law, and the optional ``leaf_mode`` key of a law's file.
"""

from fractions import Fraction

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import _capi, compiled
from tests import compiled_cpu as cc
from tests import compiled_rollout_cpu as cr
from tests import explicit_synth as es

CASES = [('nominal', 1, 1), ('noisy', 3, 2), ('guarded', 5, 4)]
_RUNS = {}


def _run(kind, p, n_u):
    """One mirror rollout per case, shared by the tests and left unchanged."""
    key = (kind, p, n_u)
    if key not in _RUNS:
        law, plant, X0, kw = cr.case(kind, p, n_u)
        arrays, _ = cc.compile_flat(law.flat)
        modes = cr.leaf_modes(law, arrays)
        mir = cr.mirror(arrays, modes, plant, X0, cr.T_STEPS, **kw)
        _RUNS[key] = (law, plant, X0, kw, arrays, modes, mir)
    return _RUNS[key]


@pytest.mark.parametrize('kind,p,n_u', CASES, ids=['%s-p%d-nu%d' % c for c in CASES])
def test_mirror_against_exact_arithmetic(kind, p, n_u):
    law, plant, X0, kw, arrays, modes, mir = _run(kind, p, n_u)
    skipped, applied = cr.check_exact(law, mir, mir.roots, mir.z, plant, modes, kw['tol_exit'])
    print('%s p%d nu%d: %d of %d applied steps skipped as non-decisive' % (kind, p, n_u, skipped,
                                                                          applied))
    assert applied > cr.N_TRAJ
    assert (mir.steps > 0).any()


@pytest.mark.parametrize('kind,p,n_u', CASES, ids=['%s-p%d-nu%d' % c for c in CASES])
def test_mirror_against_the_exact_host_rollout(kind, p, n_u):
    """Where every step of a trajectory is decisive and the chosen root's smallest exact weight
    is away from -tol_exit by more than the slack -- and not in the documented band [-tol_exit, 0)
    where the root-level and the leaf-level exit tests may differ -- steps, status and leaves are
    those of ``explicit_synth.host_rollout``."""
    law, plant, X0, kw, arrays, modes, mir = _run(kind, p, n_u)
    host = es.host_rollout(law, plant, X0, cr.T_STEPS, **kw)
    tol = Fraction(kw['tol_exit'])
    clear = np.ones(X0.shape[0], dtype=bool)
    band = 0
    for q in range(X0.shape[0]):
        for t in range(min(int(mir.steps[q]) + 1, cr.T_STEPS)):
            ref = law.locate(mir.z[t, q])
            r = int(mir.roots[t, q])
            lo = Fraction(min(law.forest.root_weights(r, ref.Y, ref.D)), ref.D)
            slack = Fraction(64 * es.EPS) * (1 + Fraction(law.kappa(r)))
            if not law.decisive(ref) or abs(lo + tol) <= slack:
                clear[q] = False
            elif -tol <= lo < 0:
                clear[q] = False
                band += 1
    print('%s p%d nu%d: %d of %d trajectories compared, %d in the band' % (
        kind, p, n_u, clear.sum(), clear.size, band))
    assert clear.sum() > clear.size // 2
    assert np.array_equal(mir.steps[clear], host.steps[clear])
    assert np.array_equal(mir.status[clear], host.status[clear])
    assert np.array_equal(mir.leaf[:, clear], host.leaf[:, clear])


def _write(path, arrays, **extra):
    with open(path, 'wb') as f:
        np.savez(f, format_version=np.int64(compiled.FORMAT_VERSION), **arrays, **extra)


def test_leaf_mode_file_key(tmp_path):
    law = es.SynthLaw(es.kuhn_forest(2), 1, 3, np.random.default_rng(3), n_sub=4)
    arrays, _ = cc.compile_flat(law.flat)
    modes = cr.leaf_modes(law, arrays)
    path = str(tmp_path / 'law.npz')
    # absent: the file loads as before
    _write(path, arrays)
    got, lm = compiled.read_file(path)
    assert lm is None and sorted(got) == sorted(arrays)
    for k in arrays:
        assert got[k].tobytes() == np.asarray(arrays[k]).tobytes(), k     # (child pairs: by bytes)
    # present
    _write(path, arrays, leaf_mode=modes)
    got, lm = compiled.read_file(path)
    assert lm.dtype == np.int32 and np.array_equal(lm, modes)
    for k in arrays:
        assert got[k].tobytes() == np.asarray(arrays[k]).tobytes(), k     # (child pairs: by bytes)
    # wrong length, a value below -1, a wrong type: refused
    low = modes.copy()
    low[0] = -2
    for bad in (modes[:-1], np.concatenate([modes, [0]]), low, modes.astype(np.float64),
                modes.reshape(1, -1)):
        _write(path, arrays, leaf_mode=bad)
        with pytest.raises(_capi.EhmError) as err:
            compiled.read_file(path)
        assert err.value.code == _capi.EHM_E_INVALID


def test_entry_points_refuse_without_a_law():
    """The rollout runs on the device or not at all: no handle, EHM_E_INVALID."""
    lib = _capi.load()
    out = [np.zeros(4), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32),
           np.zeros(2), np.zeros(2), np.zeros(2)]
    rc = lib.ehm_compiled_rollout(None, 2, 3, np.zeros(4).ctypes.data, None, None, 1e-9, None,
                                  None, None, *[a.ctypes.data for a in out], None)
    assert rc == _capi.EHM_E_INVALID
    rc = lib.ehm_compiled_rollout_noisy(None, 2, 3, np.zeros(4).ctypes.data, 0, 0, 1e-9, None,
                                        None, None, None, None, None,
                                        *[a.ctypes.data for a in out], None)
    assert rc == _capi.EHM_E_INVALID
    rc = lib.ehm_compiled_set_plant(None, 1, None, None, None, 0, None, None, None, None, 0, None,
                                    None, None, 0, None, None)
    assert rc == _capi.EHM_E_INVALID
    assert lib.ehm_compiled_set_noise(None, 0, None, None, 0, 0) == _capi.EHM_E_INVALID
