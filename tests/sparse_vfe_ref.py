"""Host restatement of the variational sparse GP (VFE, Titsias' collapsed bound; DESIGN.md
section 10), built on the DTC restatements of tests/sparse_ref.py and
tests/sparse_pseudo_ref.py:

    lZ_VFE = lZ_DTC - t / (2 sn2),    t = sum_j ( k(x_j, x_j) - |V0_j|^2 ),   V0 = L^-T Kux

and the adjoints of the trace term added to DTC's, with B0 = L^-1 V0 = (Kuu + su2 I)^-1 Kux:

    G_ux += B0 / sn2      G_uu -= B0 B0^T / (2 sn2)      g_x = -1 / (2 sn2)
    d/dlog sn:  + t / sn2  +  2 su2 tr(-B0 B0^T / (2 sn2))      (su2 = sn2 1e-6 moves with sn2)

The mean component, the posteriors and the stored factors are DTC's (sr.sparse_posterior
with sr.DTC). t is summed from per-column differences, never as sum kxx - ||V0||_F^2.
`dtype=np.longdouble` runs everything in extended precision (xprec helpers)."""

import numpy as np

from oracle import gp_oracle as orc
import sparse_pseudo_ref as spr
import sparse_ref as sr
import xprec

VFE = 3     # gpx_sparse_method; the arithmetic underneath is sr.DTC's


def trace_term(spec, theta, U, X, dtype=np.float64):
    """t, B0 (p x N), and what the contractions need: the spec with theta's hypers, U, X
    (cast to dtype), sn2, su2."""
    ld = dtype == np.longdouble
    kfun = xprec if ld else orc
    sp = sr._with_hyper(spec, theta)
    if ld:
        sp = xprec.ld_spec(sp)
    cast = (lambda a: np.asarray(a, dtype=np.longdouble)) if ld else (lambda a: a)
    U, X = cast(U), cast(X)
    sn2 = np.exp(2 * cast(theta[0]))
    su2 = sr._jitter(sr.DTC, sn2)
    p = U.shape[0]
    L = sr._chol(kfun.kernel_get(sp, U) + su2 * np.eye(p, dtype=U.dtype), ld)
    V0 = sr._solve_t(L, kfun.kernel_get(sp, U, X), ld)
    t = np.sum(kfun.kernel_dget(sp, X) - np.sum(V0 ** 2, axis=0))
    B0 = sr._solve(L, V0, ld)
    return t, B0, sp, U, X, sn2, su2


def vfe_eval(spec, theta, U, X, y, grad=True, dtype=np.float64, chunk=4096):
    """lZ (and dlZ in the layout [sn | kernel | mean]) of the VFE bound."""
    out = sr.sparse_eval(spec, sr.DTC, theta, U, X, y, grad=grad, dtype=dtype, chunk=chunk)
    t, B0, sp, U, X, sn2, su2 = trace_term(spec, theta, U, X, dtype)
    if not grad:
        return out - t / (2 * sn2)
    lZ, dlZ = out
    lZ = lZ - t / (2 * sn2)
    dlZ = dlZ.copy()
    N = X.shape[0]
    Guu = -B0.dot(B0.T) / (2 * sn2)
    dlZ[0] += t / sn2 + 2 * su2 * np.trace(Guu)
    dKuu = sr._grads(orc.kernel_grad(sp, U))
    dkxx = sr._grads(orc.kernel_dgrad(sp, X))
    gx = np.full(N, -1 / (2 * sn2), dtype=B0.dtype)
    acc = np.einsum('kij,ij->k', dKuu, Guu) + np.asarray(dkxx, dtype=B0.dtype).dot(gx)
    for j0 in range(0, N, chunk):
        sl = slice(j0, j0 + chunk)
        dKux = sr._grads(orc.kernel_grad(sp, U, X[sl]))
        acc = acc + np.einsum('kij,ij->k', dKux, B0[:, sl] / sn2)
    dlZ[1:-1] += acc
    return lZ, dlZ


def adjoints(spec, theta, U, X, y, dtype=np.float64):
    """lZ, G_uu and j0, j1 -> G_ux[:, j0:j1] of the VFE bound (spr.adjoints' layout)."""
    lZ, Guu, gux_dtc, sp, Uc, Xc = spr.adjoints(spec, sr.DTC, theta, U, X, y, dtype)
    t, B0, _, _, _, sn2, _ = trace_term(spec, theta, U, X, dtype)

    def gux(j0, j1):
        return gux_dtc(j0, j1) + B0[:, j0:j1] / sn2
    return lZ - t / (2 * sn2), Guu - B0.dot(B0.T) / (2 * sn2), gux, sp, Uc, Xc


def pseudo_grad(spec, theta, U, X, y, dtype=np.float64, chunk=4096):
    """lZ and dU = dlZ/dU (p x d): spr.pseudo_grad's contraction over the VFE adjoints
    (neither k(x, x) nor su2 depends on U)."""
    lZ, Guu, gux, sp, U, X = adjoints(spec, theta, U, X, y, dtype)
    dU = np.einsum('ij,ijc->ic', Guu + Guu.T, orc.kernel_gradx(sp, U, U))
    for j0 in range(0, X.shape[0], chunk):
        j1 = min(X.shape[0], j0 + chunk)
        dU = dU + np.einsum('ij,ijc->ic', gux(j0, j1), orc.kernel_gradx(sp, U, X[j0:j1]))
    return lZ, dU


# -- shared by tests/test_sparse_vfe_host.py and tests/test_gpu_sparse_vfe.py ---------------

def independent_t(spec, theta, U, X):
    """t (and sn2) from oracle kernel values and a dense solve: no Cholesky factor and no
    line of the restatement above."""
    sp = sr._with_hyper(spec, theta)
    sn2 = np.exp(2 * theta[0])
    Kj = orc.kernel_get(sp, U) + sn2 * 1e-6 * np.eye(len(U))
    Kux = orc.kernel_get(sp, U, X)
    return np.sum(orc.kernel_dget(sp, X) - np.sum(Kux * np.linalg.solve(Kj, Kux), axis=0)), sn2


# Gap lZ_exact - lZ_VFE of the restatement at U = X on the fixture below (SE-ARD of
# sr.FAMILIES, N = 300, sn = 0.3, mean 0.2), measured on the CPU: 6.65e-5 absolute (8.2e-7 of
# |lZ|), what the jitter leaves. The host test pins the restatement to this value and the
# device test holds the device to 10x it at the same fixture.
TIGHT_N, TIGHT_SEED, TIGHT_GAP_HOST = 300, 5, 6.65e-5


def tight_fixture():
    """desc, spec, theta, X, y of the U = X check."""
    import helpers
    desc = dict((f[0], f[1]) for f in sr.FAMILIES)['se-ard']
    rng = np.random.RandomState(TIGHT_SEED)
    X = rng.uniform(0, 5, (TIGHT_N, 3))
    y = np.sin(X[:, 0]) + 0.1 * rng.randn(TIGHT_N)
    spec = helpers.oracle_spec(desc)
    return desc, spec, np.r_[np.log(0.3), orc.spec_get_hyper(spec), 0.2], X, y
