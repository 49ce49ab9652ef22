"""
DTC sparse pseudo-input GP (pygp/inference/dtc.py) on the MI355X:
same interface (DTC(likelihood, kernel, mean, U), pseudoinputs, from_gp(gp, U),
loglikelihood, posterior, _full_posterior, _Ruu / _Rux / _a), device arithmetic in
sparse.hip.
"""

from .. import _lib
from ._sparse import SparseGP

__all__ = ['DTC']


class DTC(SparseGP):
    """GP inference using sparse pseudo-inputs (deterministic training conditional)."""

    _method = _lib.GPX_DTC

    # Ruu = chol(Kuu + su2 I), Rux = chol(Kuu + Kux Kux^T / sn2 + su2 I),
    # a = Rux^-T Kux r
    @property
    def _Ruu(self):
        return self._state(0)

    @property
    def _Rux(self):
        return self._state(1)

    @property
    def _a(self):
        return self._state(2)
