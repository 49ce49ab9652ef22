"""
pygp_amd -- MI355X-native exact-GP hot path behind pygp's Kernel / GP interface.

Only the path named in BASELINE.json is here: pairwise kernel evaluation
(SE / Matern / Periodic / RQ, sums of products), ExactGP update /
log-likelihood (+gradient) / posterior, the sparse FITC / DTC / VFE models and binary
classification by Laplace's approximation (LaplaceGP; on pseudo-inputs SparseLaplaceGP) and by
expectation propagation (EPGP; on pseudo-inputs SparseEPGP),
correlated outputs at their own inputs (CoregionalGP) and posterior function samples through
random Fourier features (FourierSample) with their regression model (SSGP) and by pathwise
conditioning on the exact solve (PathwiseSample), and matrix-free exact regression by
preconditioned conjugate gradients (IterativeGP), executed by hand-written HIP kernels in libgpx.so; `batch` and `meta` route the
per-sample loops of the reference's meta-models through the batched entry points.
"""

from . import kernels
from . import likelihoods
from . import inference
from . import learning
from . import batch
from . import meta
from .inference import (BasicGP, ExactGP, GradientGP, MultiOutputGP, CoregionalGP, LaplaceGP,
                        EPGP, MulticlassLaplaceGP, FITC, DTC, VFE, select_pseudoinputs, FourierSample, SSGP,
                        PathwiseSample, IterativeGP, SparseLaplaceGP, SparseEPGP)
from .learning import optimize

__all__ = ['BasicGP', 'ExactGP', 'GradientGP', 'MultiOutputGP', 'CoregionalGP', 'LaplaceGP', 'EPGP',
           'MulticlassLaplaceGP', 'SparseLaplaceGP', 'SparseEPGP',
           'FITC', 'DTC', 'VFE', 'select_pseudoinputs', 'FourierSample', 'SSGP', 'PathwiseSample', 'IterativeGP', 'optimize', 'kernels', 'likelihoods', 'inference', 'learning',
           'batch', 'meta']
