"""CPU reference of the transposed and the adjoint operator, from oracle pieces only.

nu and omega are real and the Green's matrix G is complex symmetric, so with ``conv`` the bare oracle convolution b -> G b

    want_T(b) = b + omega^2 nu .* conv(b)            (M^T = I + omega^2 diag(nu) G)
    want_H(b) = conj(want_T(conj(b)))                (M^H)

tests/test_adjoint_ref_cpu.py pins both against the dense A.T and A.conj().T built from ``o.mul``."""
import copy

import numpy as np

from oracle import lsfc_oracle as o


def conv_of_oracle(Mo):
    """b -> G b of an oracle operator: ``o.fft_convolution`` on a copy.  The 2D trapezoidal branch of the reference multiplies
    by nu inside its FFTconvolution, so the copy gets nu = 1 there."""
    Mc = copy.copy(Mo)
    if isinstance(Mo, o.FastM) and Mo.quadRule == "trapezoidal":
        Mc.nu = np.ones_like(np.asarray(Mo.nu, dtype=np.float64))
    return lambda b: o.fft_convolution(Mc, b)


def conv_of_reduced(G2, dims):
    """b -> G b of a plan made from the reduced symbol G2 (plain FFT order) on the grid ``dims``"""
    return lambda b: o.convolve_reduced(G2, b, dims)


def want_T(conv, nu, omega, b):
    b = np.asarray(b, dtype=np.complex128)
    return b + omega ** 2 * np.asarray(nu, dtype=np.float64) * conv(b)


def want_H(conv, nu, omega, b):
    return np.conj(want_T(conv, nu, omega, np.conj(np.asarray(b, dtype=np.complex128))))


class Ref:
    """The two references of one operator as callables (``T``, ``H``), e.g. to drive ``o.gmres``"""

    def __init__(self, conv, nu, omega):
        self.conv, self.nu, self.omega = conv, np.asarray(nu, dtype=np.float64).reshape(-1), float(omega)

    def T(self, b):
        return want_T(self.conv, self.nu, self.omega, b)

    def H(self, b):
        return want_H(self.conv, self.nu, self.omega, b)

    def of(self, which):
        return {"T": self.T, "H": self.H}[which]


def ref_of_oracle(Mo):
    return Ref(conv_of_oracle(Mo), Mo.nu, Mo.omega)
