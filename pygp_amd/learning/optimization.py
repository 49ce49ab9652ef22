"""
Type-II maximum likelihood on top of the accelerated ExactGP.

The reference's optimize() (/root/reference/pygp/learning/optimization.py:21-67)
is pure control flow over get_hyper / set_hyper / loglikelihood(True); it is
restated here only so that the drop-in can be exercised end to end
(tests/test_gpu_gp.py reproduces /root/reference/tests/test_learning.py). Each
objective call is one gpx_exact_update + one gpx_exact_loglik on the device
(objective='loo': one gpx_exact_loo, the leave-one-out log predictive probability).
"""

import numpy as np
import scipy.optimize as so

from ..utils.models import get_params

__all__ = ['optimize']


def optimize(gp, priors=None, pseudoinputs=False, objective='lik', spectrum=False):
    """Maximise the marginal likelihood over the hypers of `gp` in place.
    priors: {name: None} freezes the named block (the only prior form the
    reference supports, optimization.py:47-52). pseudoinputs: also move the
    pseudo-inputs of a sparse model (FITC, DTC, VFE), jointly with the free hypers.
    spectrum: also move the spectral points and phases of a feature model (SSGP).
    objective: 'lik' the marginal likelihood, 'loo' the leave-one-out log predictive
    probability (gp.loo, exact models only)."""
    if objective not in ('lik', 'loo'):
        raise ValueError("objective must be 'lik' or 'loo'")
    if objective == 'loo':
        if pseudoinputs:
            raise ValueError('the leave-one-out objective does not move pseudo-inputs')
        if not hasattr(gp, 'loo'):
            raise ValueError('the leave-one-out objective needs an exact model')
    if spectrum:
        if pseudoinputs or objective == 'loo':
            raise ValueError('spectrum optimisation moves no pseudo-inputs and has no '
                             'leave-one-out objective')
        return _optimize_spectrum(gp, priors)
    if pseudoinputs:
        return _optimize_pseudo(gp, priors)
    start = gp.get_hyper()
    free = np.ones(gp.nhyper, dtype=bool)
    blocks = dict((name, block) for name, block, _ in get_params(gp))
    for name, prior in (priors or {}).items():
        if prior is not None:
            raise NotImplementedError('only fixing priors (None) are supported')
        free[blocks[name]] = False

    def negative_loglik(x):
        hyper = start.copy()
        hyper[free] = x
        gp.set_hyper(hyper)
        lZ, dlZ = gp.loo(True) if objective == 'loo' else gp.loglikelihood(True)
        return -lZ, -dlZ[free]

    x, _, _ = so.fmin_l_bfgs_b(negative_loglik, start[free])
    final = start.copy()
    final[free] = x
    gp.set_hyper(final)


def _free_hypers(gp, priors):
    """(start, free): the hypers and which of them no fixing prior holds."""
    start = gp.get_hyper()
    free = np.ones(gp.nhyper, dtype=bool)
    blocks = dict((name, block) for name, block, _ in get_params(gp))
    for name, prior in (priors or {}).items():
        if prior is not None:
            raise NotImplementedError('only fixing priors (None) are supported')
        free[blocks[name]] = False
    return start, free


def _optimize_spectrum(gp, priors):
    """L-BFGS over [free hypers, S.ravel(), b]; one loglikelihood(True, spectrum=True) per
    objective call: _optimize_pseudo's twin."""
    if not hasattr(gp, 'set_spectrum'):
        raise ValueError('spectrum optimisation needs a feature model (SSGP)')
    start, free = _free_hypers(gp, priors)
    S0, b0 = gp.spectrum
    nfree, nS = int(free.sum()), S0.size

    def unpack(x):
        hyper = start.copy()
        hyper[free] = x[:nfree]
        return hyper, x[nfree:nfree + nS].reshape(S0.shape), x[nfree + nS:]

    def negative_loglik(x):
        hyper, S, b = unpack(x)
        gp.set_spectrum(S, b)            # first: set_hyper then factors once, with these
        gp.set_hyper(hyper)
        lZ, dlZ, dS, db = gp.loglikelihood(True, spectrum=True)
        return -lZ, -np.r_[dlZ[free], dS.ravel(), db]

    x, _, _ = so.fmin_l_bfgs_b(negative_loglik, np.r_[start[free], S0.ravel(), b0])
    hyper, S, b = unpack(x)
    gp.set_spectrum(S, b)
    gp.set_hyper(hyper)


def _optimize_pseudo(gp, priors):
    """L-BFGS over [free hypers, U.ravel()]; one loglikelihood(True, pseudoinputs=True)
    per objective call."""
    if not hasattr(gp, 'set_pseudoinputs'):
        raise ValueError('pseudo-input optimisation needs a sparse model (FITC, DTC, VFE)')
    start, free = _free_hypers(gp, priors)
    shape = gp.pseudoinputs.shape
    nfree = int(free.sum())

    def unpack(x):
        hyper = start.copy()
        hyper[free] = x[:nfree]
        return hyper, x[nfree:].reshape(shape)

    def negative_loglik(x):
        hyper, U = unpack(x)
        gp.set_pseudoinputs(U)           # first: set_hyper then factors once, with this U
        gp.set_hyper(hyper)
        lZ, dlZ, dU = gp.loglikelihood(True, pseudoinputs=True)
        return -lZ, -np.r_[dlZ[free], dU.ravel()]

    x, _, _ = so.fmin_l_bfgs_b(negative_loglik, np.r_[start[free], gp.pseudoinputs.ravel()])
    hyper, U = unpack(x)
    gp.set_pseudoinputs(U)
    gp.set_hyper(hyper)
