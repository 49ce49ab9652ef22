"""
Binary GP classification by Laplace's approximation (GPML algorithms 3.1, 3.2 and 5.1, with a
constant mean).

Labels y in {-1, +1} at X under a `Logistic` or `Probit` likelihood; the latent is
f = mean + K a. libgpx.so finds the mode by Newton's method -- every step one factorisation of
B = I + sW K sW^T by the exact path's code and two products with K that never store it -- and
returns the approximate log evidence lZ = Psi - sum log R_ii, its gradient in every kernel
hyperparameter and the mean, and the Gaussian approximation of the latent posterior
(gpx_laplace_*). No counterpart in the reference.
"""

from ..likelihoods import Logistic, Probit
from .. import _lib                        # noqa: F401  (the handle type of LabelsGP._dev)
from ._labels import LabelsGP

__all__ = ['LaplaceGP']


class LaplaceGP(LabelsGP):
    """Hyper layout [kernel | mean]: the likelihoods have no hyperparameter. `tol` and
    `max_iter` bound the Newton iteration (stop at max |f_new - f_old| <= tol (1 + max |f_new|);
    RuntimeError after max_iter steps). warm_start=True starts each iteration from the mode of
    the last one on the same data: fewer steps, and a result that depends on the calls before it
    to rounding; the default starts from f = mean, and the same calls give the same bits."""

    _what = 'Laplace'
    _entry = 'laplace'
    _options = ('tol', 'max_iter', 'warm_start')

    def __init__(self, likelihood, kernel, mean, tol=1e-8, max_iter=50, warm_start=False):
        if not isinstance(likelihood, (Logistic, Probit)):
            raise ValueError('Laplace inference requires a Logistic or Probit likelihood')
        super(LaplaceGP, self).__init__(likelihood, kernel, mean, tol, max_iter)
        self._warm_start = bool(warm_start)

    def _iterate(self, dev):
        """Newton's method to the mode, on the device."""
        return dev.laplace_update(self._kernel._kspec(), self._likelihood._code, self._mean,
                                  self._tol, self._max_iter, self._warm_start)

    @property
    def mode(self):
        """The mode of the latent posterior at the data, f-hat."""
        if self.ndata == 0:
            return None
        self._ensure()
        return self._dev().laplace_get_mode(self.ndata)[0]

    @property
    def newton_iterations(self):
        """Newton steps of the last update."""
        self._ensure()
        return self._iters
