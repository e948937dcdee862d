"""CPU test of the problems that tests/test_gpu_bicgstabl_multi.py compares histories on (tests/bicgstabl_multi_cases.py):
each is well enough conditioned for a comparison at 1e-10 -- the plain double-precision run with a permuted order of
summation stays within 1e-11 of the long-double run, in the history and in x, and stops at the same counts."""
import pytest

import bicgstabl_multi_cases as mc

_CASES = mc.cases()


@pytest.mark.parametrize("label", sorted(_CASES))
def test_input_condition(label):
    import bicgstabl_ref as br
    kw, _ = _CASES[label]
    dev, xdev, same, ref = br.input_condition(kw)
    print(f"{label}: history deviation {dev:.2e}, x deviation {xdev:.2e}, {ref['iters']} cycles, {ref['mvps']} mvps")
    assert same, f"{label}: the double-precision run stops elsewhere"
    assert dev < 1e-11, f"{label}: history deviates by {dev:.2e} in double precision"
    assert xdev < 1e-11, f"{label}: x deviates by {xdev:.2e} in double precision"
    if label.startswith("cap"):
        assert not ref["converged"] and ref["iters"] == 4 and ref["mvps"] == 1 + 4 * 4
    else:
        assert ref["converged"]
