"""CPU restatement of the closed loop of ehm_explicit_rollout (test infrastructure): the
reference's walk (oracle.explicit_cpu.ExplicitFlatCPU), the exit test, the plant step."""

import numpy as np

from oracle.explicit_cpu import ExplicitFlatCPU


def weights(cpu, k, z):
    """(alpha0, alpha_1..alpha_p) of z in node k."""
    a = cpu.minv(k).dot(z - cpu.V[k][0])
    return np.concatenate([[1. - a.sum()], a])


def step(cpu, plant, node_mode, x, z, tol_exit, d=None):
    """One step from the true state x seen as z: (status, leaf, u, x_next)."""
    k = cpu.get_containing_cell(z)
    lam = weights(cpu, k, z)
    if lam.min() < -tol_exit:
        return 1, k, None, None
    u = lam[0] * cpu.U[k][0] + cpu.U[k][1:].T.dot(lam[1:])
    m = int(node_mode[k])
    if m < 0:
        return 3, k, None, None
    if not plant.in_region(x[None], np.array([m]), tol_exit)[0]:
        return 2, k, u, None
    D = None if d is None else np.asarray(d)[None]
    return 0, k, u, plant.step(x[None], u[None], np.array([m]), D)[0]


def flat_cpu(flat):
    return ExplicitFlatCPU(flat.vertices, flat.vertex_inputs, flat.left, flat.right,
                           flat.info['n_roots'])
