"""
FITC sparse pseudo-input GP (pygp/inference/fitc.py) on the MI355X:
same interface (FITC(likelihood, kernel, mean, U), pseudoinputs, from_gp(gp, U),
loglikelihood, posterior, _full_posterior, _L / _R / _b), device arithmetic in sparse.hip.
"""

from .. import _lib
from ._sparse import SparseGP

__all__ = ['FITC']


class FITC(SparseGP):
    """GP inference using sparse pseudo-inputs (fully independent training conditional)."""

    _method = _lib.GPX_FITC

    # the stored statistics as the reference keeps them: L = chol(Kuu + su2 I),
    # R = chol(I + V V^T) L, b = R^-T Kux r / ell^2
    @property
    def _L(self):
        return self._state(0)

    @property
    def _R(self):
        return self._state(1)

    @property
    def _b(self):
        return self._state(2)
