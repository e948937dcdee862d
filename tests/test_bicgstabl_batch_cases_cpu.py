"""CPU tests of the problems of the lock-step batch suite (tests/bicgstabl_batch_cases.py): every member that
tests/test_gpu_bicgstabl_batch.py compares with the long-double restatement meets the input condition of
tests/test_bicgstabl_ref_cpu.py (history < 1e-11, x < 1e-12, same counts in plain double precision with another order of
summation), and the members of the "leave at different cycles" set really leave at different cycles."""
import numpy as np
import pytest

import bicgstabl_ref as br
import bicgstabl_batch_cases as bc


@pytest.mark.parametrize("l", [1, 2])
def test_leave_members_condition_and_cycles(l):
    # measured: worst history deviation 1.2e-13 (the three-entry member), worst x deviation 2.8e-16
    members = bc.leave_members(l)
    cycles = []
    for j, kw in enumerate(members):
        if not np.any(kw["b"]):
            # b == 0: nothing to compare (x == 0 exactly, no cycle): the restatement says converged at once
            ref = br.bicgstabl_ref(**kw)
            assert ref["converged"] and (ref["iters"], ref["mvps"]) == (0, 1) and not np.any(ref["x"]), j
        else:
            dev, xdev, same, ref = br.input_condition(kw)
            print(f"l={l} member {j}: {ref['iters']} cycles, history deviation {dev:.1e}, x deviation {xdev:.1e}")
            assert same, f"member {j}: the double-precision run stops elsewhere"
            assert dev < 1e-11, f"member {j}: history deviates by {dev:.2e} in double precision"
            assert xdev < 1e-12, f"member {j}: x deviates by {xdev:.2e} in double precision"
            assert ref["converged"] and ref["breakdown"] is None, j
        cycles.append(ref["iters"])
    assert tuple(cycles) == bc.LEAVE_CYCLES[l]
    assert len(set(cycles)) >= 5                         # the active list shrinks five times
    # every member stops on the shared abstol, not on its own reltol: the tolerances are per member only through beta0
    for kw in members:
        ref = br.bicgstabl_ref(**kw)
        assert ref["tol"] == bc.leave_abstol()


def test_breakdown_members():
    m0, m1 = bc.breakdown_members()
    ref = br.bicgstabl_ref(**m0)
    assert ref["breakdown"] == "sigma" and not ref["converged"] and (ref["iters"], ref["mvps"]) == (1, 3)
    assert np.array_equal(ref["resnorm"], [0.75])
    dev, xdev, same, ref = br.input_condition(m1)
    assert same and dev < 1e-11 and xdev < 1e-12
    assert ref["converged"] and (ref["iters"], ref["mvps"]) == (2, 5)
    assert np.max(np.abs(ref["x"].astype(complex) - 1.0)) < 1e-12


def test_length_members_are_distinct_right_hand_sides():
    for N in (5, 1025):
        ms = bc.length_members(N, 2)
        assert len(ms) == 3 and not np.array_equal(ms[0]["b"], ms[1]["b"]) and not np.array_equal(ms[1]["b"], ms[2]["b"])
        assert bc.stack(ms, "b", N).shape == (3, N) and not np.any(bc.stack(ms, "x0", N))
