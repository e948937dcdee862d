"""CPU reference of the operator with a complex nu (an absorbing medium), from oracle pieces only.

The reference's nu is real (``nu :: Array{Float64,1}``), but the oracle's arithmetic (``M.nu * b``) does not care: a copy of an
oracle operator whose ``nu`` is complex gives M, and with ``conv`` the bare oracle convolution b -> G b (tests/adjoint_ref.py)

    want_N(b) = b + omega^2 conv(nu .* b)            (M   = I + omega^2 G diag(nu))
    want_T(b) = b + omega^2 nu .* conv(b)            (M^T = I + omega^2 diag(nu) G, no conjugate)
    want_H(b) = conj(want_T(conj(b)))                (M^H = b + omega^2 conj(nu) .* conj(G conj(b)))

tests/test_complex_nu_ref_cpu.py pins all three against the dense A, A.T and A.conj().T."""
import copy

import numpy as np

from oracle import lsfc_oracle as o
import adjoint_ref as ar


def as_complex(nu):
    return np.ascontiguousarray(np.asarray(nu).reshape(-1), dtype=np.complex128)


def with_nu(Mo, nu):
    """a copy of the oracle operator Mo whose nu is the complex vector ``nu``"""
    Mc = copy.copy(Mo)
    Mc.nu = as_complex(nu)
    return Mc


def want_T(conv, nu, omega, b):
    b = np.asarray(b, dtype=np.complex128)
    return b + omega ** 2 * as_complex(nu) * conv(b)


def want_H(conv, nu, omega, b):
    return np.conj(want_T(conv, nu, omega, np.conj(np.asarray(b, dtype=np.complex128))))


class Ref:
    """The three references of one operator as callables (``N``, ``T``, ``H``).  ``forward``: b -> M b by the oracle's own apply
    (``o.mul`` of the copy, ``o.apply_reduced``); ``conv``: the bare convolution of the same operator."""

    def __init__(self, forward, conv, nu, omega):
        self.N, self.conv, self.nu, self.omega = forward, conv, as_complex(nu), float(omega)

    def T(self, b):
        return want_T(self.conv, self.nu, self.omega, b)

    def H(self, b):
        return want_H(self.conv, self.nu, self.omega, b)

    def of(self, which):
        return {"N": self.N, "T": self.T, "H": self.H}[which]


def ref_of_oracle(Mo, nu):
    """references of the oracle operator Mo (real nu, as the oracle builds it) with its nu replaced by the complex ``nu``"""
    Mc = with_nu(Mo, nu)
    return Ref(lambda b: o.mul(Mc, np.asarray(b, dtype=np.complex128)), ar.conv_of_oracle(Mo), nu, Mo.omega)


def ref_of_reduced(G2, dims, nu, omega):
    """references of a plan made from the reduced symbol G2 (plain FFT order) on the grid ``dims``"""
    nu = as_complex(nu)
    return Ref(lambda b: o.apply_reduced(G2, nu, omega, np.asarray(b, dtype=np.complex128), dims), ar.conv_of_reduced(G2, dims), nu, omega)


def msp_ref(built, nu, k):
    """Msp = As + k^2 AG diag(nu) from the pieces ``As`` and ``AG`` of ``sparsify_ref.build`` (whose own ``nu`` argument is cast
    to float, so it is not used with a complex nu)"""
    import scipy.sparse as sp
    return (built["As"] + k ** 2 * (built["AG"] @ sp.diags(as_complex(nu)))).tocsr()
