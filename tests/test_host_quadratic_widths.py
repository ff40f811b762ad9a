"""
The inputs of tests/test_gpu_quadratic_widths.py, checked on the CPU (no GPU needed): for every
row of helpers.QUADRATIC_WIDTH_ROWS

- the law has the size the table assumes and reaches the instance it names (the restatement of
  lp_xbase / lp_slots / k2_pick in tests/quadratic_widths_cpu.py; the GPU test asserts the same
  through ehm_problem_batch_kernel);
- condition 1: for every row slot the suboptimality-test programme occupies, some rotation has a
  reference optimum with a multiplier above 1e-6 on a row of that slot -- so a kernel that
  mishandled the rows of any slot would return another optimum;
- condition 2: the optimum does not depend on the rotation, for both references, to
  1e-9 (1 + |obj|) -- and for solve_cp to 1e-11, which lets the GPU test hold every rotation
  against the reference of the natural order at its bar of 1e-9;
- condition 3: both references converge on every input;
- the two references agree on every optimum to 1e-7 and on u0 to 1e-8: the first inputs the
  device is held to (1e-7) are well defined at these parameters;
- the parameters at 0.999 t_max are feasible and those at 1.001 t_max infeasible (HiGHS), and the
  constraints do bind: every parameter at 0.999 t_max has an active row.
"""

import numpy as np
import pytest

from tests import helpers
from tests import quadratic_widths_cpu as qw

ROWS = helpers.QUADRATIC_WIDTH_ROWS
IDS = [helpers.quadratic_width_name(r) for r in ROWS]


def rel(a, b):
    return np.max(np.abs(a - b) / (1. + np.abs(b)))


def test_layout_restatement():
    # (m, extras) -> (xbase, slots): the cases of csrc/ehm_k2.h
    assert (qw.lp_xbase(57, 7), qw.lp_slots(57, 7)) == (57, 1)        # 57 + 7 = 64: they just fit
    assert (qw.lp_xbase(58, 7), qw.lp_slots(58, 7)) == (64, 2)        # 65: a slot of their own
    assert (qw.lp_xbase(64, 5), qw.lp_slots(64, 5)) == (64, 2)        # full slot
    assert (qw.lp_xbase(250, 6), qw.lp_slots(250, 6)) == (250, 4)     # row 255 is the last
    assert (qw.lp_xbase(100, 0), qw.lp_slots(100, 0)) == (100, 2)
    assert [qw.capacity(c) for c in (1, 8, 9, 16, 17, 24, 25, 32)] == [8, 8, 16, 16, 24, 24, 32, 32]
    assert qw.rotations(6) == [0, 1] and qw.rotations(130) == [0, 1, 64, 65, 128, 129]


def test_rotation_moves_rows_only():
    row = ROWS[1]
    can = qw.law(row)
    rot = qw.rotate(can, 65)
    for i in (0, 5, can.m - 1):
        j = (i + 65) % can.m
        assert np.array_equal(rot.G[0, j], can.G[0, i]) and rot.w[0, j] == can.w[0, i]
        assert np.array_equal(rot.S[0, j], can.S[0, i])
    assert rot.H is can.H or np.array_equal(rot.H, can.H)
    assert (rot.n, rot.m, rot.p, rot.n_u) == (can.n, can.m, can.p, can.n_u)


@pytest.mark.parametrize('row', ROWS, ids=IDS)
def test_inputs_make_the_rows_matter(row):
    cap, slots, n_x, n_u, N, n_random, tag = row
    can = qw.law(row)
    n, m, p = can.n, can.m, can.p
    assert (n, m, p) == (n_u * N, N * (2 * n_x + n_random + 2 * n_u), n_x)
    assert can.quadratic and can.n_delta == 1
    assert qw.expected_instances(n, m, p)[1] == (cap, slots)
    inp = qw.inputs(row)
    assert inp.theta.shape == (qw.N_DIRECTIONS * len(qw.POINT_FRACTIONS), p)
    for th in inp.inside:
        assert qw.feasible_highs(can, th)
    for th in inp.outside:
        assert not qw.feasible_highs(can, th)
    ref0 = qw.reference(row, 0)
    # the two references against each other, natural order
    for a, b in ((ref0.pt, ref0.pt_qp), (ref0.sl, ref0.sl_qp), (ref0.ms, ref0.ms_qp)):
        assert rel(a, b) <= 1e-7
    assert np.abs(ref0.u0 - ref0.u0_qp).max() <= qw.U0_REF_TOL
    # the rows bind near the boundary
    active = np.array(ref0.n_active).reshape(qw.N_DIRECTIONS, len(qw.POINT_FRACTIONS))
    assert (active[:, -1] >= 1).all(), active
    hit = set()
    worst_cp = worst_qp = 0.
    for shift in qw.rotations(m):
        ref = qw.reference(row, shift)
        assert ref.ok, shift                                                     # condition 3
        hit |= ref.slots_hit
        for name in ('pt', 'sl', 'ms', 'vbar'):
            worst_cp = max(worst_cp, rel(getattr(ref, name), getattr(ref0, name)))
        for name in ('pt_qp', 'sl_qp', 'ms_qp'):
            worst_qp = max(worst_qp, rel(getattr(ref, name), getattr(ref0, name)))
    print('\n%s: n %d m %d p %d, %d rotations, slots hit %s of %d, active rows per parameter %s, '
          'rotation changes solve_cp by %.1e, qp_numpy by %.1e'
          % (helpers.quadratic_width_name(row), n, m, p, len(qw.rotations(m)), sorted(hit), slots,
             ref0.n_active, worst_cp, worst_qp))
    assert hit == set(range(slots))                                              # condition 1
    assert worst_cp <= 1e-11 and worst_qp <= 1e-9                                # condition 2
