"""
Variational sparse pseudo-input GP (VFE: Titsias' collapsed bound, the objective of sparse
GP regression) on the MI355X. The reference has no such class; the interface is DTC's
(VFE(likelihood, kernel, mean, U), pseudoinputs, from_gp(gp, U), loglikelihood, posterior,
_full_posterior, _Ruu / _Rux / _a), and so are the posterior and the stored statistics.
loglikelihood is a lower bound of the exact GP's for every U,

    lZ = lZ_DTC - sum_j (k(x_j, x_j) - q_jj) / (2 sn2),    Q = Kxu (Kuu + su2 I)^-1 Kux,

which makes it the objective to move pseudo-inputs with (optimize(gp, pseudoinputs=True)).
Device arithmetic in sparse.hip.
"""

from .. import _lib
from ._sparse import SparseGP

__all__ = ['VFE']


class VFE(SparseGP):
    """GP inference using sparse pseudo-inputs (variational free energy)."""

    _method = _lib.GPX_VFE

    # DTC's statistics: Ruu = chol(Kuu + su2 I),
    # Rux = chol(Kuu + Kux Kux^T / sn2 + su2 I), a = Rux^-T Kux r
    @property
    def _Ruu(self):
        return self._state(0)

    @property
    def _Rux(self):
        return self._state(1)

    @property
    def _a(self):
        return self._state(2)
