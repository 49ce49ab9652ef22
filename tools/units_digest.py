#!/usr/bin/env python3
"""One line per call with a digest of what it returned, for a refactor that moves code between
units without changing what it computes. Covers every entry that reaches the kernel-matrix units
(pygp_amd/csrc/kmat.hip, kgrad.hip, kderiv.hip): input widths on both sides of the 8 / 16 / 32
instances, ragged sizes that span tile edges, every kernel family; and every family of the C ABI's
units (pygp_amd/csrc/gpx_*.hip), with a refused call per family on a handle in another state (the
refusal's text is part of the line) and one pass over the exact-path families at N = 2100, the
smallest order that takes the blocked driver with lead rows, the look-ahead streams and the
split-k route of the posterior's products. Run it from two trees (it imports the package of the
tree it lies in) on the same device: the outputs must not differ. The last line counts the
arrays and the doubles.
The routes of the task-queue launches (pygp_amd/csrc/panel.hip, panel_graph.hip) at the smallest
shapes that take them: a whole matrix in one launch with its right-hand side, without and with
the whole inverse (N = 300, three tiles, one panel; N = 1100, nine tiles); the member-batched
launch (6 thetas) and the lock-step sweep (16 and 33 thetas), value-only and with gradients; the
blocked driver's wide panels in the N = 2100 pass. `panel` runs these alone, for a pass per
developer switch (GPX_PANEL_STRICT, GPX_PANEL_SPLIT, GPX_PANEL_STREAM, GPX_SWEEP_LITE,
GPX_SOLO_MAX_NP / GPX_SOLO_MIN_MEMBERS).
usage: units_digest.py [panel] > out.txt"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pygp_amd import _lib, kernels as K

WIDTHS = (1, 8, 9, 16, 17, 32)
N1, N2, MS = 129, 70, (4, 130)
NBIG, DBIG = 2100, 4
LSN, MEAN = np.log(0.1), 0.2
# CoregionalGP, T = 3: uneven task counts, B = L L^T, a noise and a mean per task
ICM_T = 3
ICM_L = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [-0.3, 0.4, 0.7]])
ICM_B = ICM_L @ ICM_L.T
ICM_LSN = np.log([0.1, 0.2, 0.15])
ICM_MEAN = np.array([0.2, -0.1, 0.3])
count = [0, 0]


def dig(*arrays):                                   # as tools/jitter_check.py
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return h.hexdigest()[:16]


def families(d):
    ell = 0.5 * np.sqrt(d) * (1.0 + 0.1 * np.arange(d))
    out = [('se_iso', K.SE(1.1, 0.6 * np.sqrt(d), ndim=d)), ('se_ard', K.SE(1.1, ell)),
           ('matern3', K.Matern(0.9, ell, d=3)), ('matern5', K.Matern(1.2, ell, d=5)),
           ('rq', K.RQ(1.1, ell, 1.5)), ('sum', K.SE(0.8, ell) + K.Matern(0.6, 1.3 * ell, d=5)),
           ('product', K.SE(1.1, 1.5 * ell) * K.RQ(0.9, 2.0 * ell, 2.0))]
    if d == 1:
        out.append(('periodic', K.Periodic(1.1, 0.8, 0.7)))
    return out


def tasks(n):                                       # 0, 1, 2 at 3 : 2 : 2
    return (np.arange(n) % 7 % ICM_T).astype(np.int32)


def put(tag, call):
    try:
        res = call()
    except Exception as e:                           # a refusal is a result too
        print('%-44s refused: %s' % (tag, str(e).split('\n')[0][:80]), flush=True)
        return
    arrays = [np.asarray(a, dtype=np.float64) for a in (res if isinstance(res, tuple) else (res,))]
    count[0] += len(arrays)
    count[1] += sum(a.size for a in arrays)
    print('%-44s %s %d' % (tag, dig(*arrays), sum(a.size for a in arrays)), flush=True)


def exact_families(h, t, spec, nh, X, y, Y3, Xg, G, ngo, Xs):
    """The four families that ride the exact pipeline, on the data given: ngo values beside the
    gradients G at Xg; Xs: {m: test points}, a few and more than a tile of them."""
    few, many = sorted(Xs)
    n = X.shape[0]

    def plain():
        h.set_data(X, y)
        h.exact_update(spec, LSN, MEAN)
        return (h.exact_loo(nh, n, grad=True) + h.exact_loo(nh, n, points=True)
                + h.exact_posterior_full(Xs[few]) + h.exact_get_factor(n))

    def multiout():                                  # MultiOutputGP, T = 3
        h.mo_set_data(X, Y3)
        h.mo_update(spec, LSN, MEAN)
        return h.mo_loglik(nh, True) + h.mo_posterior(Xs[many]) + h.mo_posterior_full(Xs[few])

    def gradobs():                                   # GradientGP
        h.gradobs_set_data(X[:ngo], y[:ngo], Xg, G)
        h.gradobs_update(spec, LSN, 0.05, MEAN)
        return ((h.gradobs_loglik(),) + h.gradobs_posterior(Xs[many])
                + h.gradobs_posterior_full(Xs[few]))

    def coregional():                                # CoregionalGP
        h.icm_set_data(X, y, tasks(n), ICM_T)
        h.icm_update(spec, ICM_LSN, ICM_B, ICM_MEAN)
        return (h.icm_loglik(nh, True) + h.icm_posterior(Xs[many], tasks(many))
                + h.icm_posterior_full(Xs[few], tasks(few)))

    put(t('exact loo / full / factor'), plain)
    put(t('multiout'), multiout)
    put(t('gradobs'), gradobs)
    put(t('coregional'), coregional)


def refusals(h, t, spec, nh, X, y, labels, Xs):
    """Every family's entries on a handle that holds another family's data, or its own without an
    update."""
    m = sorted(Xs)[0]
    h.laplace_set_data(X, labels)                    # labels: the exact-path families refuse
    put(t('exact_update on labels'), lambda: h.exact_update(spec, LSN, MEAN))
    put(t('exact_eval on labels'), lambda: h.exact_eval(spec, LSN, MEAN, True))
    put(t('kernel_build_resident on labels'), lambda: h.kernel_build_resident(spec))
    put(t('mo_update on labels'), lambda: h.mo_update(spec, LSN, MEAN))
    put(t('gradobs_update on labels'), lambda: h.gradobs_update(spec, LSN, 0.05, MEAN))
    put(t('icm_update on labels'), lambda: h.icm_update(spec, ICM_LSN, ICM_B, ICM_MEAN))
    put(t('sparse_update on labels'), lambda: h.sparse_update(spec, _lib.GPX_FITC, X[:20], LSN, MEAN))
    put(t('laplace_loglik, no update'), lambda: h.laplace_loglik(nh, True))
    put(t('ep_posterior, no update'), lambda: h.ep_posterior(Xs[m]))
    h.set_data(X, y)                                 # plain data: the others refuse
    put(t('laplace_update on plain'), lambda: h.laplace_update(spec, 2, MEAN))
    put(t('ep_update on plain'), lambda: h.ep_update(spec, MEAN))
    put(t('mo_loglik on plain'), lambda: h.mo_loglik(nh, True))
    put(t('gradobs_posterior on plain'), lambda: h.gradobs_posterior(Xs[m]))
    put(t('icm_loglik on plain'), lambda: h.icm_loglik(nh, True))
    put(t('exact_loglik, no update'), lambda: h.exact_loglik(nh, True))
    put(t('exact_loo, no update'), lambda: h.exact_loo(nh, X.shape[0], grad=True))
    put(t('exact_posterior, no update'), lambda: h.exact_posterior(Xs[m]))
    put(t('exact_get_factor, no update'), lambda: h.exact_get_factor(X.shape[0]))
    h.mo_set_data(X, np.c_[y, y * y])
    put(t('mo_loglik, no update'), lambda: h.mo_loglik(nh, True))
    put(t('exact_loglik on multiout'), lambda: h.exact_loglik(nh, True))
    h.gradobs_set_data(X[:40], y[:40], X[40:45], np.ones((5, X.shape[1])))
    put(t('gradobs_loglik, no update'), lambda: h.gradobs_loglik())
    put(t('loglik_batch on gradobs'), lambda: h.loglik_batch(spec, np.zeros((2, nh + 2)), grad=True))
    h.icm_set_data(X, y, tasks(X.shape[0]), ICM_T)
    put(t('icm_loglik, no update'), lambda: h.icm_loglik(nh, True))
    put(t('icm_posterior, no update'), lambda: h.icm_posterior(Xs[m], tasks(m)))
    put(t('exact_append on coregional'), lambda: h.exact_append(X[:2], y[:2]))


def panel_routes(h):
    d = 3
    k = K.SE(1.1, 0.5 * np.sqrt(d) * (1.0 + 0.1 * np.arange(d)))
    spec, hyp, nh = k._kspec(), k.get_hyper(), k.nhyper
    for n in (300, 1100):
        rng = np.random.RandomState(500 + n)
        X = rng.rand(n, d)
        y = np.sin(3 * X.sum(axis=1)) + 0.1 * rng.randn(n)
        t = lambda what: 'N=%-4d panel    %s' % (n, what)
        h.set_data(X, y)
        put(t('exact_eval value'), lambda: h.exact_eval(spec, LSN, MEAN, False))
        put(t('exact_eval grad'), lambda: h.exact_eval(spec, LSN, MEAN, True))
        for B in (6, 16, 33):
            base = np.r_[LSN, hyp, MEAN]
            thetas = base + 0.1 * np.cos(np.arange(B * (nh + 2)).reshape(B, nh + 2))
            for grad in (False, True):              # (the plan of the batch names its route)
                plan = h.batch_plan(B, grad)
                put(t('loglik_batch B=%d %s, %s x %d' % (B, 'grad' if grad else 'value', plan['arrangement'],
                                                         plan['members_per_group'])),
                    lambda: h.loglik_batch(spec, thetas, grad=grad))


ONLY_PANEL = sys.argv[1:] == ['panel']
h = _lib.Handle(0)
panel_routes(h)
for d in () if ONLY_PANEL else WIDTHS:
    rng = np.random.RandomState(1000 + d)
    X, X2 = rng.rand(N1, d), rng.rand(N2, d)
    Xs = {m: rng.rand(m, d) for m in MS}
    y = np.sin(3 * X.sum(axis=1)) + 0.1 * rng.randn(N1)
    Y3 = np.c_[y, np.cos(2 * X[:, 0]), y * y]
    labels = np.where(y > np.median(y), 1.0, -1.0)
    V = rng.randn(N1, 3)
    ng = 9
    Xg, G = rng.rand(ng, d), rng.randn(ng, d)
    Xnew, ynew = rng.rand(5, d), rng.randn(5)
    for name, k in families(d):
        spec, hyp, nh = k._kspec(), k.get_hyper(), k.nhyper
        t = lambda what: 'd=%-2d %-8s %s' % (d, name, what)
        thetas = np.array([np.r_[LSN, hyp, MEAN], np.r_[LSN, hyp, MEAN] + 0.1 * np.cos(np.arange(nh + 2))])
        # the kernel entries
        put(t('kernel_get f64'), lambda: h.kernel_get(spec, X, X2))
        put(t('kernel_get f64 square'), lambda: h.kernel_get(spec, X))
        put(t('kernel_get f32'), lambda: h.kernel_get(spec, X, X2, dtype=np.float32))
        put(t('kernel_grad'), lambda: h.kernel_grad(spec, X, X2))
        put(t('kernel_gradx wrt 1'), lambda: h.kernel_gradx(spec, X, X2, wrt=1))
        put(t('kernel_gradx wrt 2'), lambda: h.kernel_gradx(spec, X, X2, wrt=2))
        put(t('kernel_gradxy'), lambda: h.kernel_gradxy(spec, X2, X2[:33]))
        put(t('kernel_matvec'), lambda: h.kernel_matvec(spec, X, V))
        # ExactGP and the member-batched group
        h.set_data(X, y)
        put(t('select_pivots'), lambda: h.select_pivots(spec, X, 20))
        # (the call's result is a time: that it ran is what the line says)
        put(t('kernel_build_resident f32'),
            lambda: 0.0 * h.kernel_build_resident(spec, dtype=np.float32, reps=1))
        put(t('exact_eval grad'), lambda: h.exact_eval(spec, LSN, MEAN, True))
        put(t('exact_update'), lambda: (h.exact_update(spec, LSN, MEAN), h.exact_loglik(nh, True))[1])
        for m in MS:
            put(t('exact_posterior_grad m=%d' % m), lambda: h.exact_posterior_grad(Xs[m]))
            put(t('exact_posterior_gradient m=%d' % m), lambda: h.exact_posterior_gradient(Xs[m]))
        put(t('exact_append'), lambda: (float(h.exact_append(Xnew, ynew)),) + h.exact_posterior_grad(Xs[4]))
        h.set_data(X, y)
        put(t('loglik_batch grad'), lambda: h.loglik_batch(spec, thetas, grad=True))
        put(t('posterior_batch grad'), lambda: h.posterior_batch(spec, thetas, Xs[4], grad=True))

        def sparse(method):                          # 70 pseudo-inputs, with their gradients
            h.sparse_update(spec, method, X2, LSN, MEAN)
            return (h.sparse_loglik(nh, True) + h.sparse_loglik_pseudo(nh, N2, d)
                    + h.sparse_posterior(Xs[4], grad=True))

        def laplace():                               # LaplaceGP, Probit
            h.laplace_set_data(X, labels)
            steps = h.laplace_update(spec, 2, MEAN)
            return ((float(steps),) + h.laplace_loglik(nh, True) + h.laplace_posterior(Xs[130])
                    + h.laplace_get_mode(N1) + h.laplace_posterior_full(Xs[4]))

        def ep():                                    # EPGP on the same labels
            sweeps = h.ep_update(spec, MEAN)
            return ((float(sweeps),) + h.ep_loglik(nh, True) + h.ep_posterior(Xs[130])
                    + h.ep_get_sites(N1) + h.ep_posterior_full(Xs[4]))

        exact_families(h, t, spec, nh, X, y, Y3, Xg, G, 40, Xs)
        h.set_data(X, y)
        for mname, method in (('fitc', _lib.GPX_FITC), ('dtc', _lib.GPX_DTC), ('vfe', _lib.GPX_VFE)):
            put(t(mname), lambda: sparse(method))
        put(t('laplace'), laplace)
        put(t('ep'), ep)
    refusals(h, t, spec, nh, X, y, labels, Xs)

# the exact-path families where the factorisation is blocked: one width, two kernels
rng = np.random.RandomState(77)
X = rng.rand(NBIG, DBIG)
y = np.sin(3 * X.sum(axis=1)) + 0.1 * rng.randn(NBIG)
Y3 = np.c_[y, np.cos(2 * X[:, 0]), y * y]
Xs = {m: rng.rand(m, DBIG) for m in MS}
ng = 25                                              # 2000 values + 25 x 4 gradients: order 2100
Xg, G = rng.rand(ng, DBIG), rng.randn(ng, DBIG)
for name, k in families(DBIG)[1:3]:
    spec, nh = k._kspec(), k.nhyper
    t = lambda what: 'N=%d %-8s %s' % (NBIG, name, what)
    h.set_data(X, y)
    put(t('exact_eval grad'), lambda: h.exact_eval(spec, LSN, MEAN, True))
    put(t('exact_update'), lambda: (h.exact_update(spec, LSN, MEAN), h.exact_loglik(nh, True))[1])
    for m in MS:
        put(t('exact_posterior_grad m=%d' % m), lambda: h.exact_posterior_grad(Xs[m]))
    exact_families(h, t, spec, nh, X, y, Y3, Xg, G, NBIG - ng * DBIG, Xs)

# the dense building blocks at ragged sizes (they overwrite the handle's GP state)
rng = np.random.RandomState(78)
S = rng.randn(300, 300)
put('la_potrf n=300 inverse', lambda: h.la_potrf(S @ S.T + 300 * np.eye(300), inverse=True))
M_, N_, K_ = 256, 384, 640                            # (the engine takes whole tiles only)
lda, ldb, ldc = K_ + 32, N_ + 32, N_ + 32
put('la_gemm_ex 256 x 384 x 640, padded rows',
    lambda: h.la_gemm_ex(rng.randn(M_ * lda), rng.randn(K_ * ldb), rng.randn(M_ * ldc), M=M_, N=N_,
                         K=K_, lda=lda, ldb=ldb, ldc=ldc, alpha=-0.7, beta=1.0)[0])
h.close()
print('%d arrays, %d doubles' % tuple(count))
