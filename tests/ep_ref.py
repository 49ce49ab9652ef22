"""Reference for EPGP (binary classification by expectation propagation, GPML sections 3.6 and
5.5.2 with a constant mean m, Probit likelihood) in NumPy / SciPy: kernel matrices from the
oracle's `get` / `grad` (oracle/gp_oracle.py), the parallel iteration of the device in float64
and in np.longdouble (tests/xprec.py; the Probit moments in longdouble come from the Mills ratio
below), and an independent sequential EP (GPML algorithm 3.5: one site at a time, rank-one
update of Sigma).

Labels y in {-1, +1}, prior f ~ N(m 1, K), sites in natural parameters tau_i >= 0 and nu_i,
nu' = nu - tau m, sW = sqrt tau, B = I + sW K sW^T = R^T R. Derived here, not copied:

  posterior  prod_i exp(-tau_i f_i^2 / 2 + nu_i f_i) N(f; m, K) in g = f - m has the linear term
             nu' and the precision K^-1 + diag tau: Sigma = K - K sW B^-1 sW K,
             mu - m = Sigma nu' = K b with b = nu' - sW o B^-1 (sW o K nu').
             sW Sigma sW = I - B^-1, so Sigma_ii = (1 - (B^-1)_ii) / tau_i with
             (B^-1)_ii = sum_j (R^-1)_ij^2.
  cavity     tc = 1 / Sigma_ii - tau, vc = mu_i / Sigma_ii - nu; s2c = 1 / tc, muc = vc / tc.
  moments    of Phi(y f) N(f; muc, s2c): z = y muc / sqrt(1 + s2c), Z = Phi(z), r = N(z) / Phi(z),
             mean muc + y s2c r / sqrt(1 + s2c), variance s2c (1 - w), w = s2c r (z + r) / (1 + s2c).
  new site   tau_new = 1 / (s2c (1 - w)) - tc = tc w / (1 - w),
             nu_new = mean / variance - vc = tc (muc w + y s2c r / sqrt(1 + s2c)) / (1 - w).
  weak sites tau_i >= FLOOR / K_ii on tau_new and on the damped result (the device's rule).
  sweep      all sites from the same marginals, tau <- (1 - eta) tau + eta tau_new (nu alike),
             then the marginals again; stop when max(max |tau_new - tau|, max |nu_new - nu|) <=
             tol (1 + max(max tau, max |nu|)) BEFORE the step: the sites, the marginals and the
             factor of that pass are then one consistent set, and lZ is taken from it.
  evidence   lZ = log int N(f; m, K) prod_i Zt_i exp(-tau_i f_i^2 / 2 + nu_i f_i) df with the
             site's scale Zt_i matching the zeroth moment. In the site's moment form
             (s2t = 1 / tau, mut = nu / tau), GPML (3.65, 3.73) with the mean m:
               -1/2 log |K + St| - 1/2 (mut - m)^T (K + St)^-1 (mut - m) + sum log Phi(z)
               + 1/2 sum log(s2c + s2t) + sum (muc - mut)^2 / (2 (s2c + s2t))       [lZ_definition]
             |K + St| = |B| / prod tau and log(s2c + s2t) = log1p(tau / tc) - log tau: the
             log tau cancel and leave -sum log R_ii + 1/2 sum log1p(tau / tc).
             (K + St)^-1 = T - T Sigma T (T = diag tau) and mut - m = nu' / tau: the first
             quadratic form is -1/2 sum nu'^2 / tau + 1/2 nu'^T (mu - m). With vc' = vc - tc m,
             muc - mut = vc' / tc - nu' / tau, and -nu'^2 / (2 tau) joins the last term per point
             to ((tau / tc) vc'^2 - 2 vc' nu' - nu'^2) / (2 (tc + tau)): nothing divides by
             tau.                                                                  [lZ_stable]
             tests/test_ep_host.py holds the two forms together in longdouble.
  gradient   lZ is stationary in the sites at a fixed point (GPML 5.5.2), so only K's explicit
             part counts: d lZ / d theta = 1/2 sum_ij (b_i b_j - Wt_ij) dK_ij,
             Wt = sW sW^T o B^-1; d lZ / d m = sum b.
  prediction mu* = m + k*^T b, V = R^-T (sW o k*), s2* = k** - |V|^2, Sigma* = K** - V^T V,
             p(y = +1) = Phi(mu* / sqrt(1 + s2*)).
"""

import numpy as np
import scipy.linalg as sla

import laplace_ref as lr
import xprec
from oracle import gp_oracle as orc

LD = np.longdouble
MEAN = lr.MEAN
MS = (4, 130)                    # test-point counts of the GPU checks
FLOOR = 1e-10                    # GPX_EP_FLOOR of pygp_amd/csrc/gpx_labels.hip
TOL, MAX_ITER, DAMPING = 1e-10, 200, 0.8


# -- the Probit moments ---------------------------------------------------------------------------

def _mills(t):
    """(1 - Phi(t)) / N(t) for t >= 0 in longdouble: below 2 from the series
    Phi(t) - 1/2 = N(t) sum_k t^(2k+1) / (2k+1)!! (positive terms; the difference
    sqrt(pi / 2) exp(t^2 / 2) - sum loses a factor 22 at most), from 2 on the continued
    fraction 1 / (t + 1 / (t + 2 / (t + ...))) evaluated from its 400th term."""
    t = np.asarray(t, dtype=LD)
    out = np.empty_like(t)
    lo = t < 2
    if np.any(lo):
        x = t[lo]
        term, s = x.copy(), x.copy()
        for k in range(1, 80):
            term = term * x * x / (2 * k + 1)
            s = s + term
        out[lo] = np.sqrt(orc._PI_LD / 2) * np.exp(x * x / 2) - s
    if np.any(~lo):
        x = t[~lo]
        f = x.copy()
        for k in range(400, 0, -1):
            f = x + k / f
        out[~lo] = 1 / f
    return out


def probit_moments(z, dtype=float):
    """(log Phi(z), r = N(z) / Phi(z)): float64 in the forms of the device (lik_point in
    pygp_amd/csrc/lik_dev.h, through tests/laplace_ref.py), longdouble from the Mills ratio."""
    z = np.asarray(z, dtype=dtype)
    if dtype is not LD:
        lp, r, _, _ = lr.lik_terms('probit', np.ones(z.shape), z)
        return lp, r
    M = _mills(np.abs(z))
    logN = -z * z / 2 - np.log(2 * orc._PI_LD) / 2
    neg = z < 0
    tail = np.exp(logN) * M                              # 1 - Phi(|z|)
    lp = np.where(neg, logN + np.log(M), np.log1p(-np.where(neg, 0, tail)))
    r = np.where(neg, 1 / M, np.exp(logN) / (1 - np.where(neg, 0, tail)))
    return lp, r


def cavity(Sii, mu, tau, nu):
    tc = 1 / Sii - tau
    vc = mu / Sii - nu
    return tc, vc


def site_pass(y, Sii, mu, tau, nu, tfloor, dtype=float):
    """New sites from the marginals: (tau_new, nu_new, tc, vc, z, log Phi(z))."""
    tc, vc = cavity(Sii, mu, tau, nu)
    s2c, muc = 1 / tc, vc / tc
    den = np.sqrt(1 + s2c)
    z = y * muc / den
    lp, r = probit_moments(z, dtype)
    w = s2c * r * (z + r) / (1 + s2c)
    tn = np.maximum(tc * w / (1 - w), tfloor)
    vn = tc * (muc * w + y * s2c * r / den) / (1 - w)
    return tn, vn, tc, vc, z, lp


# -- dense pieces in either precision ----------------------------------------------------------

def _rinv(R, dtype):
    if dtype is LD:
        return xprec.tri_inverse(R)
    return sla.solve_triangular(R, np.eye(len(R)), lower=False)


def marginals(K, tau, nu, mean, dtype=float):
    """(R, R^-1, sW, nu', b, mu, Sigma_ii) of the sites; tau > 0."""
    sW = np.sqrt(tau)
    R = lr._chol(np.eye(len(K), dtype=dtype) + sW[:, None] * K * sW[None, :], dtype)
    Ri = _rinv(R, dtype)
    nup = nu - tau * mean
    x = Ri @ (Ri.T @ (sW * (K @ nup)))
    b = nup - sW * x
    mu = mean + K @ b
    Sii = (1 - np.sum(Ri * Ri, axis=1)) / tau
    return R, Ri, sW, nup, b, mu, Sii


def lZ_stable(R, tau, nu, mu, tc, vc, lp, mean):
    """The evidence in the form of the device: nothing divides by tau."""
    nup, vcp = nu - tau * mean, vc - tc * mean
    return (-np.sum(np.log(np.diag(R))) + np.sum(np.log1p(tau / tc)) / 2 + np.sum(lp)
            + nup @ (mu - mean) / 2
            + np.sum(((tau / tc) * vcp ** 2 - 2 * vcp * nup - nup ** 2) / (2 * (tc + tau))))


def lZ_definition(K, tau, nu, tc, vc, lp, mean, dtype=LD):
    """The evidence in the site's moment form (see the module's text), with its own Cholesky of
    K + diag(1 / tau)."""
    s2t, mut = 1 / tau, nu / tau
    s2c, muc = 1 / tc, vc / tc
    L = lr._chol(K + np.diag(s2t), dtype)
    a = lr._solve(L, mut - mean, True, dtype)
    return (-np.sum(np.log(np.diag(L))) - a @ a / 2 + np.sum(lp)
            + np.sum(np.log(s2c + s2t)) / 2 + np.sum((muc - mut) ** 2 / (2 * (s2c + s2t))))


def _finish(out, grad):
    """lZ, and with grad the gradient, from the consistent set of a fit."""
    dtype, K, tau = out['dtype'], out['K'], out['tau']
    out['lZ'] = lZ_stable(out['R'], tau, out['nu'], out['mu'], out['tc'], out['vc'], out['lp'],
                          out['mean'])
    if grad:
        Ri, sW, b = out['Ri'], out['sW'], out['b']
        Wt = sW[:, None] * (Ri @ Ri.T) * sW[None, :]
        Q = np.outer(b, b) - Wt
        sp_ = lr._spec(out['spec'], dtype)
        dlZ = [np.sum(Q * G) / 2 for G in orc.kernel_grad(sp_, out['X'])]
        out.update(Wt=Wt, dlZ=np.array(dlZ + [np.sum(b)], dtype=dtype))
    return out


def fit(spec, mean, X, y, tol=TOL, max_iter=MAX_ITER, damping=DAMPING, dtype=float, grad=True):
    """Damped parallel EP as the device runs it, and everything at its fixed point. `sweeps`
    counts the damped steps taken; more than max_iter is a RuntimeError."""
    X, y = np.array(X, ndmin=2, dtype=dtype), np.asarray(y, dtype=dtype)
    n = len(X)
    mean, eta = dtype(mean), dtype(damping)
    sp_ = lr._spec(spec, dtype)
    K = orc.kernel_get(sp_, X)
    tfloor = dtype(FLOOR) / np.diag(K)
    tau, nu = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    Sii, mu = np.diag(K).copy(), np.full(n, mean, dtype=dtype)
    state = None
    sweeps = 0
    while True:
        tn, vn, tc, vc, z, lp = site_pass(y, Sii, mu, tau, nu, tfloor, dtype)
        change = max(np.max(np.abs(tn - tau)), np.max(np.abs(vn - nu)))
        if not np.isfinite(change):
            raise FloatingPointError('the sites left the numbers at sweep %d' % sweeps)
        if state is not None and change <= tol * (1 + max(np.max(tau), np.max(np.abs(nu)))):
            break
        if sweeps == max_iter:
            raise RuntimeError('no convergence in %d sweeps' % max_iter)
        sweeps += 1
        tau = np.maximum(tau + eta * (tn - tau), tfloor)
        nu = nu + eta * (vn - nu)
        state = marginals(K, tau, nu, mean, dtype)
        mu, Sii = state[5], state[6]
    R, Ri, sW, nup, b, mu, Sii = state
    out = dict(spec=spec, mean=mean, X=X, y=y, dtype=dtype, K=K, tau=tau, nu=nu, R=R, Ri=Ri, sW=sW,
               b=b, g=b, mu=mu, Sii=Sii, tc=tc, vc=vc, z=z, lp=lp, sweeps=sweeps)
    return _finish(out, grad)


def fit_sequential(spec, mean, X, y, tol=TOL, max_iter=MAX_ITER, dtype=float, grad=False):
    """GPML algorithm 3.5: the sites one at a time, undamped, Sigma and mu by rank-one updates and
    afresh from the sites after every sweep; the stopping rule over a sweep's changes."""
    X, y = np.array(X, ndmin=2, dtype=dtype), np.asarray(y, dtype=dtype)
    n = len(X)
    mean = dtype(mean)
    K = orc.kernel_get(lr._spec(spec, dtype), X)
    tfloor = dtype(FLOOR) / np.diag(K)
    tau, nu = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    Sigma, mu = K.copy(), np.full(n, mean, dtype=dtype)
    for sweeps in range(1, max_iter + 1):
        change = 0
        scale = 1 + max(np.max(tau), np.max(np.abs(nu)))
        for i in range(n):
            one = slice(i, i + 1)
            tn, vn = site_pass(y[one], Sigma[i, one], mu[one], tau[one], nu[one], tfloor[one],
                               dtype)[:2]
            dtau, dnu = tn[0] - tau[i], vn[0] - nu[i]
            change = max(change, abs(dtau), abs(dnu))
            tau[i], nu[i] = tn[0], vn[0]
            si = Sigma[:, i].copy()
            # Sigma_new = Sigma - dtau / (1 + dtau Sigma_ii) s_i s_i^T; mu - m = Sigma_new nu'_new
            Sigma = Sigma - (dtau / (1 + dtau * si[i])) * np.outer(si, si)
            mu = mean + Sigma @ (nu - tau * mean)
        R, Ri, sW, nup, b, mu, Sii = marginals(K, tau, nu, mean, dtype)
        Sigma = K - (K * sW[None, :]) @ (Ri @ Ri.T) @ (sW[:, None] * K)
        if change <= tol * scale:
            break
    else:
        raise RuntimeError('no convergence in %d sweeps' % max_iter)
    tc, vc = cavity(Sii, mu, tau, nu)
    z = y * (vc / tc) / np.sqrt(1 + 1 / tc)
    out = dict(spec=spec, mean=mean, X=X, y=y, dtype=dtype, K=K, tau=tau, nu=nu, R=R, Ri=Ri, sW=sW,
               b=b, g=b, mu=mu, Sii=Sii, tc=tc, vc=vc, z=z, lp=probit_moments(z, dtype)[0],
               sweeps=sweeps)
    return _finish(out, grad)


def lZ_at(spec, theta, X, y, dtype=LD, tol=1e-17):
    """lZ at the hypers theta = [kernel | mean] (for differences of lZ)."""
    sp_ = orc.spec_set_hyper(orc._deepcopy_spec(spec), np.asarray(theta[:-1], dtype=float))
    if dtype is LD:
        sp_ = xprec.spec_with_hyper(spec, np.asarray(theta[:-1], dtype=LD))
    return fit(sp_, theta[-1], X, y, tol=tol, max_iter=400, dtype=dtype, grad=False)['lZ']


def posterior(ref, Xs):
    """(mu, s2, Sigma) of the latent f at the rows of Xs: Laplace's with g -> b."""
    return lr.posterior(ref, Xs)


def predict(mu, s2):
    return lr.predict('probit', mu, s2)


# -- inputs ---------------------------------------------------------------------------------------

problem = lr.problem
family = lr.family
NS = (1, 2, 37, 129, 257)        # the GPU sizes: one point, two, a ragged tile, the 128-tile
D = 3                            # crossed by one, a third tile row
FAMILIES = ('se_ard', 'matern5', 'sum', 'product')


def cases():
    """(family, n) of the GPU comparison."""
    return [(name, n) for name in FAMILIES for n in NS]


def hard_problem(n=129):
    """(descriptor, mean, X, y): labels separable by a plane in [0, 2]^3 under sf = 30 and a mean
    on the wrong side of one class. Undamped parallel EP needs far more than 50 sweeps on it;
    damping 0.8 converges in about 40."""
    X = 2 * np.random.RandomState(129).rand(n, D)
    y = np.where(X.sum(axis=1) > D, 1.0, -1.0)
    return ('se', (30.0, np.linspace(0.6, 1.4, D)), {}), 5.0, X, y


def cluster_problem():
    """The hard case of tests/laplace_ref.py: two separable clusters on a line, sf = 30, m = 5.
    The sites of a cluster are so strongly coupled that parallel EP at damping 0.8 ends in a
    cycle of period two; 0.5 converges (about 100 sweeps)."""
    return lr.hard_problem()


def weak_problem(n=37):
    """(descriptor, mean, X, y): every label +1 under m = 50 and sf = 1: z = 50 / sqrt 2 at
    every point, the new precisions are of the size exp(-z^2 / 2) = 1e-272 and every site sits
    at the floor. Without the floor 1 - (B^-1)_ii rounds to zero and Sigma_ii is 0 / 0."""
    X = 2 * np.random.RandomState(11).rand(n, D)
    return ('se', (1.0, np.linspace(0.6, 1.4, D)), {}), 50.0, X, np.ones(n)
