"""
Binary GP classification by expectation propagation (GPML sections 3.6 and 5.5.2, with a
constant mean).

Labels y in {-1, +1} at X under the `Probit` likelihood, whose moments against a Gaussian are
closed forms. Every label gets a Gaussian site in natural parameters (tau_i >= 0, nu_i);
libgpx.so runs EP in its parallel form -- one sweep updates all sites from their cavities at
once, damped, and then costs what a Newton step of LaplaceGP costs: one factorisation of
B = I + sW K sW^T (sW = sqrt tau) by the exact path's code, two products with K that never
store it, and the diagonal of the posterior covariance from the rows of R^-1 -- and returns the
EP approximation of the log evidence, its gradient in every kernel hyperparameter and the mean,
and the Gaussian approximation of the latent posterior (gpx_ep_*). No
counterpart in the reference.
"""

from ..likelihoods import Logistic, Probit
from ._labels import LabelsGP

__all__ = ['EPGP']


class EPGP(LabelsGP):
    """Hyper layout [kernel | mean]. `tol` and `max_iter` bound the sweeps (stop at
    max(max |tau_new - tau|, max |nu_new - nu|) <= tol (1 + max(max tau, max |nu|)) before the
    damped step; RuntimeError after max_iter sweeps); `damping` in (0, 1] is the share of the new
    site a sweep takes: undamped parallel EP oscillates on separable labels under a large signal
    variance, 0.8 converged on everything tried. Every update starts from
    zero sites: the same calls give the same bits."""

    _what = 'EP'
    _entry = 'ep'
    _options = ('tol', 'max_iter', 'damping')

    def __init__(self, likelihood, kernel, mean, tol=1e-10, max_iter=200, damping=0.8):
        if isinstance(likelihood, Logistic):
            raise ValueError('EP inference requires the Probit likelihood: the moments of a '
                             'Logistic likelihood against a Gaussian have no closed form, and '
                             'their quadrature is not built')
        if not isinstance(likelihood, Probit):
            raise ValueError('EP inference requires the Probit likelihood')
        damping = float(damping)
        if not 0 < damping <= 1:
            raise ValueError('damping must be in (0, 1]')
        super(EPGP, self).__init__(likelihood, kernel, mean, tol, max_iter)
        self._damping = damping

    def _iterate(self, dev):
        """Damped parallel EP to a fixed point of the sites, on the device."""
        return dev.ep_update(self._kernel._kspec(), self._mean, self._tol, self._max_iter,
                             self._damping)

    @property
    def sites(self):
        """(tau, nu): the natural parameters of the sites at the fixed point."""
        if self.ndata == 0:
            return None
        self._ensure()
        return self._dev().ep_get_sites(self.ndata)[:2]

    @property
    def sweeps(self):
        """Sweeps of the last update."""
        self._ensure()
        return self._iters
