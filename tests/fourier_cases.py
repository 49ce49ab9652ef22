"""The cases of tests/golden/g_fourier.npz, shared by its generator
(tests/golden/make_golden_fourier.py) and the tests: kernel descriptors and data recipes of
tests/recipes.py, the number of features, the noise, the mean and the seed of each case."""

import numpy as np

import recipes

# name -> (kernel descriptor, input width, data, features, sn, mean, seed)
# data 'small': the 10 points of recipes.inference_points (g_small's recipe); 'mid': the 200
# points of recipes.synthetic with 10 test points; 'none': a prior sample at the small points
CASES = {}
for _i, _k in enumerate(['se_ard', 'se_iso', 'matern_ard1', 'matern_ard3', 'matern_ard5']):
    CASES['small.' + _k] = (recipes.SMALL_KERNELS[_k], 2, 'small', 100, 0.5, 0.1, 11 + _i)
for _i, _k in enumerate(['se_ard8', 'se_iso3', 'matern1_ard8', 'matern3_ard8', 'matern5_ard16']):
    CASES['mid.' + _k] = (recipes.MID_CASES[_k][0], recipes.MID_CASES[_k][1], 'mid', 129, 0.1,
                          0.25, 21 + _i)
CASES['none.se_ard'] = (recipes.SMALL_KERNELS['se_ard'], 2, 'none', 100, 0.5, 0.1, 31)


def case_data(name):
    """(X, y, Xs) of a case; X and y are None without data."""
    _, D, data, _, sn, _, _ = CASES[name]
    if data == 'mid':
        return recipes.synthetic(recipes.MID_N, D, n_test=10)
    X, y, Xs, _ = recipes.inference_points(D, np.log(sn))
    return (None, None, Xs) if data == 'none' else (X, y, Xs)


def case_sf(name):
    """The signal amplitude of the case's kernel (every case is one stationary part)."""
    return float(CASES[name][0][1][0])
