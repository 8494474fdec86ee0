"""A kept ``_BlockPass`` (``emg3d_amd/_blockpass.py``): ``gauss_newton_solve`` runs all its
Hessian products, and with ``precondition='data'`` all its preconditioner applications, on ONE pass object whose scratch
buffers every product uses again. Here that reuse is held against one-shot calls and fresh passes, bit for bit: the same
kernels run in the same order on the same bits, whatever the buffers held before.

The small survey comes from ``test_sensitivity``, with two frequencies; the diagonal regulariser from
``test_data_preconditioner``; device helpers from ``test_reciprocal``.
"""
import functools

import numpy as np
import pytest

from emg3d_amd import gradient
from test_data_preconditioner import DIAGONAL
from test_reciprocal import _dev
from test_sensitivity import OPTS, RECS, SRCS, TOL, _random_data, small_model

FREQS2 = {'f': 1.0, 'g': 2.5}
KEEPS = ['device', 'host']


@functools.lru_cache(maxsize=None)
def _survey(keep):
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS2, RECS, solver_opts=OPTS, tol_gradient=TOL, keep=keep)
    return grid, rec.forward()


def _weights(rec, zero_g=False):
    """Data weights in [0.1, 2]; ``zero_g``: all zero on frequency 'g', which every product then skips."""
    rng = np.random.default_rng(5)
    W = {p: rng.uniform(0.1, 2.0, len(RECS)) for p in rec.pairs}
    if zero_g:
        for p in rec.pairs:
            if p[1] == 'g':
                W[p][:] = 0.0
    return W


def _blocks(rec, grid, K, count, seed=7):
    rng = np.random.default_rng(seed)
    return [rec.to_device(rng.standard_normal((K, 1) + tuple(grid.shape_cells))) for _ in range(count)]


@pytest.mark.gpu
@pytest.mark.parametrize('zero_g', [False, True], ids=['all-frequencies', 'g-skipped'])
@pytest.mark.parametrize('keep', KEEPS)
def test_kept_pass_gives_the_bits_of_one_shot_calls(keep, zero_g):
    """K = 3 in groups of 2 (a ragged last group): J^T W J on V1, V2 and V1 again through one pass, each the bits of a
    fresh ``hessian_vec_block``; with weights that vanish on 'g' that frequency is skipped and leaves nothing stale."""
    import torch
    grid, rec = _survey(keep)
    W = _weights(rec, zero_g)
    V1, V2 = _blocks(rec, grid, 3, 2)
    ps = rec._pass(_dev(), 3, 2, rec._check_weights(W))
    for V in (V1, V2, V1):
        got = rec._gradient_block(ps.hessian_vec(V))
        assert set(ps.wdevs) == ({'f'} if zero_g else {'f', 'g'})
        assert float(got.abs().max()) > 0
        assert torch.equal(got, rec.hessian_vec_block(V, W, on_device=True, columns_per_pass=2))


def _preconditioned(rec, K, kc):
    """The set-up of ``_data_preconditioner`` for K dampings and the diagonal regulariser: the ``_BlockPCG`` with its
    kept pass, set-up dict and table, and the checked weights."""
    import torch
    dev = _dev()
    n, ncell = gradient._NCOMP[rec.model.case], rec.model.grid.n_cells
    w = rec._check_weights(_weights(rec))
    pcg = rec._pcg(dev, torch.zeros((K, n, ncell), dtype=torch.float64, device=dev), np.array([0.3, 30.0])[:K], kc, w,
                   rec._regulariser_geometry(None, dev), rec._check_regulariser(**DIAGONAL), None, 'data')
    return pcg, w


@pytest.mark.gpu
@pytest.mark.parametrize('kc', [1, 8])
@pytest.mark.parametrize('keep', KEEPS)
def test_interleaved_products_do_not_leak(keep, kc):
    """A Hessian product and a preconditioner application take turns on one pass, twice, as in the solve with
    ``precondition='data'``, where they share every buffer: each result is the bits of the same product on a fresh pass."""
    import torch
    grid, rec = _survey(keep)
    pcg, w = _preconditioned(rec, 2, kc)
    V, U = _blocks(rec, grid, 2, 2, seed=11)

    def hessian(ps):
        return rec._gradient_block(ps.hessian_vec(V))

    def application(ps):
        return rec._gradient_block(ps.precondition(U, pcg.pre, pcg.table))
    for _ in range(2):
        for product in (hessian, application):
            got = product(pcg.ps)
            assert float(got.abs().max()) > 0
            assert torch.equal(got, product(rec._pass(_dev(), 2, kc, w)))


@pytest.mark.gpu
@pytest.mark.parametrize('keep', KEEPS)
def test_kept_pass_allocates_nothing_after_its_first_use(keep):
    """After a warm-up product, with every result deleted: the bytes that torch has allocated are the same after the
    second and after the third product -- for the Hessian product, the preconditioner application and J^T y."""
    import torch
    grid, rec = _survey(keep)
    pcg, w = _preconditioned(rec, 2, 8)
    V, = _blocks(rec, grid, 2, 1)
    Y = [_random_data(np.random.default_rng(k), rec.pairs, len(RECS)) for k in range(2)]
    products = {'hessian_vec': lambda ps: ps.hessian_vec(V),
                'precondition': lambda ps: ps.precondition(V, pcg.pre, pcg.table), 'jtvec': lambda ps: ps.jtvec(Y)}
    for name, product in products.items():
        ps, held = rec._pass(_dev(), 2, 8, w), []
        for _ in range(3):
            out = rec._gradient_block(product(ps))
            del out
            torch.cuda.synchronize()
            held.append(torch.cuda.memory_allocated())
        assert held[1] == held[2], (name, held)


@pytest.mark.gpu
@pytest.mark.parametrize('keep', KEEPS)
def test_jtvec_with_gaps_on_a_kept_pass(keep):
    """K = 4 data sets in groups of 2; column 1 has no datum at 'f', column 2 only NaN at 'g': the columns that are left
    make a gap at 'f' (0, 2 | 3). Twice on one pass: the bits of ``jtvec_block``."""
    import torch
    grid, rec = _survey(keep)
    rng = np.random.default_rng(13)
    Y = [_random_data(rng, rec.pairs, len(RECS)) for _ in range(4)]
    for p in rec.pairs:
        if p[1] == 'f':
            del Y[1][p]
        else:
            Y[2][p][:] = np.nan
    want = rec.jtvec_block(Y, on_device=True, columns_per_pass=2)
    assert all(float(want[k].abs().max()) > 0 for k in range(4))
    ps = rec._pass(_dev(), 4, 2)
    for _ in range(2):
        assert torch.equal(rec._gradient_block(ps.jtvec(Y)), want)
