"""MI355X-native fast-convolution operator and GMRES for the Lippmann-Schwinger
equation: the FastM / FastM3D hot path of tanderson92/Fast_solver_Lippmann_Schwinger
behind the reference's own operator surface.  See DESIGN.md and include/lsfc.h."""
from .operators import (FastM, FastM3D, OperatorView, ConvergenceHistory, FFTconvolution, buildFastConvolution,
                        buildFastConvolution3D, eltype, fastconvolution, gmres_, gmres_batch_, bicgstabl_, bicgstabl_multi_, bicgstabl_batch_, apply_batch, mul_, profile_apply,
                        referenceValsTrapRule, sampleG3D, sampleGConv, size, time_apply)
from .preconditioner import SparsifyingPreconditioner
from .receivers import Receivers
from .born import BornOperator, born_contract
from .sparsify import (buildSparseA, buildSparseAG, buildSparseAConv, buildSparseAGConv, buildSparseA3DConv,
                       buildSparseAG3DConv, sparsifying_pair, sparsify_arrays, sparsify_pattern)
from ._lib import LsfcError, device_count, load, host_register, host_unregister, host_empty

__all__ = ["FastM", "FastM3D", "OperatorView", "ConvergenceHistory", "FFTconvolution", "buildFastConvolution",
           "buildFastConvolution3D", "eltype", "fastconvolution", "gmres_", "gmres_batch_", "bicgstabl_", "bicgstabl_multi_", "bicgstabl_batch_", "apply_batch", "mul_", "profile_apply",
           "referenceValsTrapRule", "sampleG3D", "sampleGConv", "size", "time_apply", "LsfcError",
           "device_count", "load", "SparsifyingPreconditioner", "Receivers", "BornOperator", "born_contract", "host_register", "host_unregister", "host_empty",
           "buildSparseA", "buildSparseAG", "buildSparseAConv", "buildSparseAGConv", "buildSparseA3DConv",
           "buildSparseAG3DConv", "sparsifying_pair", "sparsify_arrays", "sparsify_pattern"]
