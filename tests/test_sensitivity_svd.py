"""Randomised truncated SVD of the weighted sensitivity: the two kernels of ``csrc/orthonormal.h``
(``emg3d_dev_block_gram``, ``emg3d_dev_block_rotate``) through the C ABI against NumPy in ``longdouble``, the
orthonormalisation built on them (``ReciprocalSensitivity.orthonormalise_block``) against prescribed blocks, and
``ReciprocalSensitivity.sensitivity_svd`` against ``numpy.linalg.svd`` of the dense matrix built row by row from ``jtvec``.

The bounds. ``block_gram``: ``(n + 16) eps sum_k |y_i[k] y_j[k]|`` per entry, the project's bound for a sum in any order;
the inputs have little cancellation (values in [0.5, 1.5]) and every chunk's partial is asserted, from the reference
alone, to be at least 100 bounds, so a dropped chunk cannot hide. ``block_rotate``: ``(ncol_in + 2) eps sum_i |y_i[k] t[i,
j]|``. Orthonormalisation: the span within ``2 (K + 2) sqrt(K) eps (kappa + 1)`` (derived at the test), ``max |Q^T Q - I|``
within 16 times that of Householder QR on the same block. Method, exact case: Weyl and the triangle inequality with
``E``, the error of ``B = W^1/2 J^ Q`` from the entrywise bound ``test_block_products`` has for ``jvec_block`` (1e-10 of the
max-norm per pair); truncated case: twice the expectation bound of Halko, Martinsson and Tropp (SIAM Review 53, 2011),
Corollary 10.10.

Inputs, the small survey and the recorder come from ``test_sensitivity``, device helpers from ``test_reciprocal``. Figures
that the tests observe are printed and, with ``EMG3D_AMD_PARITY_FILE`` set, appended to that file
(``profiles/sensitivity_svd_parity.txt`` is such a run).
"""
import functools

import numpy as np
import pytest

import emg3d_amd as emg3d
from emg3d_amd import _lib, gradient
from emg3d_amd._blockpass import _svqb_rotation
from test_reciprocal import _comp_grid, _dev, _up
from test_sensitivity import EPS, FREQS, OPTS, RECS, SRCS, TOL, record, small_model

LD = np.longdouble
SYMBOLS = ('emg3d_block_gram_ws_len', 'emg3d_dev_block_gram', 'emg3d_dev_block_rotate')
NONE = {'forward': 0, 'receiver': 0, 'jvec': 0, 'jtvec': 0}
CHUNK = 4096                              # elements per partial of k_block_gram
TILE = 4                                  # its tile of column pairs
FINAL = 256                               # threads of k_block_gram_final: partial i is added by thread i % 256
MARGIN = 100.0                            # min |partial| >= MARGIN * bound: the condition on the inputs


def _message(call, kind=ValueError):
    with pytest.raises(kind) as err:
        call()
    return str(err.value)


# ----------------------------------------------------------------------- not gpu tests ---
def test_declared_symbols_and_public_methods():
    header = open(_lib.HEADER).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name) and name + '(' in header
    for name in ('orthonormalise_block', 'sensitivity_svd'):
        assert callable(getattr(gradient.ReciprocalSensitivity, name))
        assert not hasattr(gradient.Sensitivity, name)


@pytest.mark.parametrize('case, n', [('isotropic', 1), ('VTI', 2)])
def test_arguments_are_validated_before_any_gpu_work(case, n):
    """Every bad ``rank``, ``oversample``, ``power_iterations``, ``seed``, ``weights`` and ``columns_per_pass``, a sketch
    wider than 64 columns, and every bad block of ``orthonormalise_block``: ``ValueError`` with "Provided:", raised
    without a device; a Laplace-domain and a mixed survey: ``NotImplementedError``. Nothing has been solved or kept."""
    import torch
    grid, model = small_model(case)
    shape = tuple(grid.shape_cells)
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    for bad in (0, -1, 2.0, None, True, '3'):
        assert "`rank` must be an integer >= 1" in _message(lambda: rec.sensitivity_svd(bad))
    for name in ('oversample', 'power_iterations', 'seed'):
        for bad in (-1, 1.5, None, True):
            text = _message(lambda: rec.sensitivity_svd(4, **{name: bad}))
            assert f"`{name}` must be an integer >= 0" in text and "Provided:" in text
    for bad in (0, -1, 2.0, None, True):
        assert "`columns_per_pass` must be an integer >= 1" in _message(lambda: rec.sensitivity_svd(4, columns_per_pass=bad))
    nrec = len(RECS)
    for w in ({('a', 'f'): -np.ones(nrec)}, {('a', 'f'): np.ones(nrec + 1)}, {('a', 'f'): 1j * np.ones(nrec)}):
        text = _message(lambda: rec.sensitivity_svd(4, weights=w))
        assert text == _message(lambda: rec.hessian_diagonal(w)) and "Provided:" in text
    # M = 2 x 2 x 17 = 68 data rows: a sketch of more than 64 columns is possible, and refused
    many = np.array([[x, 10., -40., 0., 0.] for x in np.linspace(-60., 70., 17)])
    wide = gradient.ReciprocalSensitivity(model, SRCS, FREQS, many)
    text = _message(lambda: wide.sensitivity_svd(60, oversample=5))
    assert "must not exceed 64" in text and "Provided: 65" in text
    good = (n,) + shape
    bad_blocks = [np.zeros((0,) + good), np.zeros((2, n + 1) + shape), np.zeros(good[1:]), np.zeros((2,) + good, dtype=complex),
                  np.float64(1.0)]
    for bad in bad_blocks:
        text = _message(lambda: rec.orthonormalise_block(bad))
        assert "`vectors` must be real with shape" in text and "Provided:" in text
    for bad in (torch.zeros((2, n, grid.n_cells), dtype=torch.float64), torch.zeros((2, n, grid.n_cells), dtype=torch.float32)):
        assert "a device block must be a contiguous float64 tensor" in _message(lambda: rec.orthonormalise_block(bad))
    text = _message(lambda: rec.orthonormalise_block(np.zeros((65,) + good)))
    assert "must not exceed 64" in text and "Provided: 65" in text
    for freqs in ({'f': -1.0}, {'f': 1.0, 'g': -2.0}):
        lap = gradient.ReciprocalSensitivity(model, SRCS, freqs, RECS)
        assert "frequency-domain surveys only" in _message(lambda: lap.sensitivity_svd(4), NotImplementedError)
        assert lap.n_solves == NONE and lap.kept_bytes == 0
    assert rec.n_solves == NONE and rec.kept_bytes == 0 and wide.n_solves == NONE and wide.kept_bytes == 0


def test_no_cpu_fallback_without_gpu():
    if _lib.lib().emg3d_device_count() > 0:
        pytest.skip("GPU present")
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    v = np.ones((2,) + tuple(grid.shape_cells))
    for call in (lambda: rec.sensitivity_svd(4), lambda: rec.orthonormalise_block(v)):
        assert "no HIP device" in _message(call, _lib.Emg3dAmdError)


# ------------------------------------------------------- blocks with prescribed singular values ---
ORTH_SHAPE, ORTH_K = (19, 6, 7), 12
ORTH_BLOCKS = {'cond 1': (1.0, 12), 'cond 1e3': (1e3, 12), 'cond 1e6': (1e6, 12), 'two equal columns': (1e3, 11)}
ORTH_FACTOR = 16.0                        # over Householder QR: both are O(K eps), with different constants


@functools.lru_cache(maxsize=None)
def _orth_block(name):
    """(K, 3, 19, 6, 7): K model vectors of a triaxial model whose flattened (N, K) matrix has the singular values
    ``logspace(0, -log10 cond, K)``; 'two equal columns': vector 5 is vector 2. With it the flattened matrix (N, K), the
    singular values of what was built and ``max |Q^T Q - I|`` of Householder QR on it."""
    cond, rank = ORTH_BLOCKS[name]
    rng = np.random.default_rng(ORTH_K + int(np.log10(cond)))
    N = 3 * int(np.prod(ORTH_SHAPE))
    left, _ = np.linalg.qr(rng.standard_normal((N, ORTH_K)))
    right, _ = np.linalg.qr(rng.standard_normal((ORTH_K, ORTH_K)))
    Y = (left * np.logspace(0, -np.log10(cond), ORTH_K)) @ right.T
    if rank < ORTH_K:
        Y[:, 5] = Y[:, 2]
    qh, _ = np.linalg.qr(Y)
    householder = float(np.max(np.abs(qh.T @ qh - np.eye(ORTH_K))))
    sv = np.linalg.svd(Y, compute_uv=False)
    return np.ascontiguousarray(Y.T).reshape((ORTH_K, 3) + ORTH_SHAPE), Y, sv, householder


def _span_bound(sv, rank):
    """``|Y - Q Q^T Y|_F / |Y|_F`` for ``Q = (Y T1) T2``: the span of ``Y T`` is that of ``Y`` for ANY T of full rank, so
    only the rounding of the two rotations counts. An entry of a rotation errs by at most ``(K + 2) eps sum_i |y_i[k]|
    |t_ij| <= (K + 2) eps |y[k, :]|_2 |t[:, j]|_2``, the block by ``(K + 2) eps |Y|_F |T|_F``, and mapped back by the
    inverse of T on the kept directions that is ``(K + 2) eps sqrt(K) kappa(T) |Y|_F`` with ``kappa(T) = kappa(Y)`` (``Y T``
    is orthonormal), kappa over the ``rank`` kept singular values; the second rotation starts from kappa = 1. Twice that,
    for the terms of second order."""
    K = len(sv)
    return 2 * (K + 2) * np.sqrt(K) * EPS * (sv[0] / sv[rank - 1] + 1)


@pytest.mark.parametrize('name', list(ORTH_BLOCKS))
def test_the_orth_blocks_stay_within_the_cap_in_numpy(name):
    """The condition on the chosen blocks, on the CPU: a NumPy model of the two SVQB passes (Gram matrix by ``@``, the
    library's own ``_svqb_rotation``, rotation by ``@``) finds the expected rank, stays within 16 times Householder's
    ``max |Q^T Q - I|`` and within the span bound -- before the GPU tests rely on either."""
    _, Y, sv, householder = _orth_block(name)
    Q = Y
    for _ in range(2):
        Q = Q @ _svqb_rotation(Q.T @ Q)
    rank = Q.shape[1]
    orth = float(np.max(np.abs(Q.T @ Q - np.eye(rank))))
    span = float(np.linalg.norm(Y - Q @ (Q.T @ Y)) / np.linalg.norm(Y))
    record(f"orthonormalise, NumPy model, {name}: rank {rank}; max |Q^T Q - I| = {orth:.2e}, Householder QR {householder:.2e} "
           f"(cap {ORTH_FACTOR:.0f} x); span {span:.2e} (bound {_span_bound(sv, rank):.2e})")
    assert rank == ORTH_BLOCKS[name][1]
    assert orth <= ORTH_FACTOR * householder
    assert span <= _span_bound(sv, rank)


def test_svqb_rotation_reveals_the_rank():
    """A zero block has rank 0, a zero column is dropped, and scaling a column by 1e150 changes nothing but its row of T."""
    assert _svqb_rotation(np.zeros((3, 3))).shape == (3, 0)
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((40, 4))
    Y[:, 1] = 0.0
    T = _svqb_rotation(Y.T @ Y)
    assert T.shape == (4, 3) and np.all(T[1] == 0.0)
    Z = Y.copy()
    Z[:, 2] *= 1e150
    Q = Z @ _svqb_rotation(Z.T @ Z)
    assert Q.shape == (40, 3) and np.max(np.abs(Q.T @ Q - np.eye(3))) <= 1e-13


# ------------------------------------------------------------------ kernels on the gpu ---
N_SIZES = [1, 5, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17]
NCOLS = [1, 2, TILE, TILE + 1, 9, 33, 64]
LAYOUTS = ['aligned', 'odd']              # rows on 16-byte boundaries (16-byte loads) or on an odd stride (element-wise)


def _block(rng, rows, n, layout, positive):
    """(rows, stride) float64 with stride > n and NaN behind every row, which must never be read."""
    stride = n + 2 + n % 2 if layout == 'aligned' else (n + 3 + rows) | 1
    a = np.full((rows, stride), np.nan)
    a[:, :n] = rng.uniform(0.5, 1.5, (rows, n)) if positive else rng.standard_normal((rows, n))
    return a, stride


def _gram(Yd, stride, n, ncol, check=True, bad=()):
    """G (ncol, ncol) and the workspace after ``emg3d_dev_block_gram``; both start as NaN."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    ws = torch.full((max(L.emg3d_block_gram_ws_len(n, ncol), 1),), float('nan'), dtype=torch.float64, device=_dev())
    G = torch.full((ncol * ncol,), float('nan'), dtype=torch.float64, device=_dev())
    args = dict(n=n, ncol=ncol, y=_ptr(Yd), stride=stride, g=_ptr(G), ws=_ptr(ws))
    args.update(dict(bad))
    status = L.emg3d_dev_block_gram(args['n'], args['ncol'], args['y'], args['stride'], args['g'], args['ws'], _stream())
    if not check:
        torch.cuda.synchronize()
        return status, G.cpu().numpy()
    _lib.check(status, 'emg3d_dev_block_gram')
    return G.cpu().numpy().reshape(ncol, ncol), ws.cpu().numpy()


def _gram_reference(Y, n):
    """In longdouble: G, the bound ``(n + 16) eps sum_k |y_i y_j|`` and per entry the smallest chunk partial."""
    Yl = Y[:, :n].astype(LD)
    starts = list(range(0, n, CHUNK))
    parts = np.stack([Yl[:, s:s + CHUNK] @ Yl[:, s:s + CHUNK].T for s in starts])
    mag = np.abs(Yl) @ np.abs(Yl).T
    return parts.sum(axis=0), (n + 16) * EPS * mag.astype(float), np.min(np.abs(parts), axis=0).astype(float), len(starts)


def _check_gram(tag, Y, stride, n, ncol):
    want, bound, least, nchunk = _gram_reference(Y, n)
    assert np.all(least >= MARGIN * bound)                       # the inputs: no chunk's partial can hide in the bound
    assert _lib.lib().emg3d_block_gram_ws_len(n, ncol) == ncol * ncol * nchunk
    Yd = _up(Y)
    got, ws = _gram(Yd, stride, n, ncol)
    assert not np.any(np.isnan(got))
    ratio = np.abs(got - want) / bound
    record(f"block_gram {tag}: {nchunk} partials per entry, passes of the final loop: {-(-nchunk // FINAL)}; min |partial| / "
           f"bound = {float(np.min(least / bound)):.2e} (needs {MARGIN:.0f}); max |diff| / bound = {float(np.max(ratio)):.2e} "
           f"(bound (n + 16) eps)")
    assert np.all(ratio <= 1)
    assert np.array_equal(got, got.T)                            # symmetric bit for bit
    again, ws2 = _gram(Yd, stride, n, ncol)
    assert np.array_equal(got, again) and np.array_equal(ws, ws2, equal_nan=True)
    assert np.array_equal(Yd.cpu().numpy(), Y, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('ncol', NCOLS)
@pytest.mark.parametrize('n', N_SIZES)
def test_block_gram_vs_numpy(n, ncol, layout):
    """``|G[i, j] - want| <= (n + 16) eps sum_k |y_i[k] y_j[k]|`` against longdouble for one element, one ragged pack, one
    chunk - 1 / exactly / + 1 and three chunks + 17, by 1, 2, one tile, one tile + 1, 9, 33 and 64 columns, rows on 16-byte
    boundaries and on an odd stride; NaN lies behind every row. ``G == G.T`` bit for bit; a second call gives the same
    bits (workspace included); the block is left as it was."""
    rng = np.random.default_rng(1000 * ncol + n + (layout == 'odd'))
    Y, stride = _block(rng, ncol, n, layout, positive=True)
    _check_gram(f"n={n} ncol={ncol} {layout}", Y, stride, n, ncol)


@pytest.mark.gpu
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('n', [FINAL * CHUNK, FINAL * CHUNK + 1])
def test_block_gram_final_past_one_pass(n, layout):
    """256 partials per entry, the last size with one pass of ``k_block_gram_final``, and 257, the last of them from a
    chunk of ONE element, which thread 0 adds in its second round; two columns."""
    rng = np.random.default_rng(n + (layout == 'odd'))
    Y, stride = _block(rng, 2, n, layout, positive=True)
    _check_gram(f"n={n} ncol=2 {layout}", Y, stride, n, 2)


def _rotate(Yd, stride, n, nin, nout, Td, out_stride, check=True, bad=()):
    """out (nout, out_stride) after ``emg3d_dev_block_rotate``; it starts as NaN."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    out = torch.full((nout, out_stride), float('nan'), dtype=torch.float64, device=_dev())
    args = dict(n=n, nin=nin, nout=nout, y=_ptr(Yd), stride=stride, t=_ptr(Td), out=_ptr(out), out_stride=out_stride)
    args.update(dict(bad))
    status = _lib.lib().emg3d_dev_block_rotate(args['n'], args['nin'], args['nout'], args['y'], args['stride'], args['t'],
                                               args['out'], args['out_stride'], _stream())
    if not check:
        torch.cuda.synchronize()
        return status, out.cpu().numpy()
    _lib.check(status, 'emg3d_dev_block_rotate')
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('nin, nout', [(1, 1), (5, 3), (9, 9), (64, 17)])
@pytest.mark.parametrize('n', N_SIZES)
def test_block_rotate_vs_numpy(n, nin, nout, layout):
    """``|out_j[k] - want| <= (ncol_in + 2) eps sum_i |y_i[k] t[i, j]|`` against longdouble; every element of a row of
    ``out`` is written and the padding, preset to NaN, is still NaN; ``Y`` is left as it was; a second call gives the
    same bits. (64, 17): two tiles of outputs, the second ragged."""
    rng = np.random.default_rng(100 * nin + nout + n + (layout == 'odd'))
    Y, stride = _block(rng, nin, n, layout, positive=False)
    T = rng.standard_normal((nin, nout))
    out_stride = n + 4 + n % 2 if layout == 'aligned' else (n + 5) | 1
    Yd, Td = _up(Y), _up(T)
    got = _rotate(Yd, stride, n, nin, nout, Td, out_stride)
    want = T.T.astype(LD) @ Y[:, :n].astype(LD)
    bound = (nin + 2) * EPS * (np.abs(T).T @ np.abs(Y[:, :n]))
    assert not np.any(np.isnan(got[:, :n])) and np.all(np.isnan(got[:, n:]))
    worst = float(np.max(np.abs(got[:, :n] - want) / bound))
    record(f"block_rotate n={n} ({nin}, {nout}) {layout}: max |diff| / bound = {worst:.2e} (bound (ncol_in + 2) eps)")
    assert np.all(np.abs(got[:, :n] - want) <= bound)
    assert np.array_equal(Yd.cpu().numpy(), Y, equal_nan=True) and np.array_equal(Td.cpu().numpy(), T)
    assert np.array_equal(got, _rotate(Yd, stride, n, nin, nout, Td, out_stride), equal_nan=True)


@pytest.mark.gpu
def test_block_entries_refuse_bad_arguments():
    """Null pointers, sizes and column counts out of range, strides below a row and overlapping blocks:
    ``EMG3D_ERR_BADARG`` (-1) with the entry's name, before anything is launched (the output is still NaN); the good
    calls pass."""
    L = _lib.lib()
    assert L.emg3d_block_gram_ws_len(3 * CHUNK + 17, 9) == 81 * 4
    assert all(L.emg3d_block_gram_ws_len(*bad) == 0 for bad in ((0, 1), (5, 0), (5, -1), (5, 65)))
    rng = np.random.default_rng(8)
    n, ncol = 40, 3
    Y, stride = _block(rng, 65, n, 'aligned', positive=True)
    Yd, Td = _up(Y), _up(rng.standard_normal((65, 65)))
    from emg3d_amd._device import _ptr
    for bad in (dict(y=None), dict(g=None), dict(ws=None), dict(n=0), dict(ncol=0), dict(ncol=-2), dict(ncol=65),
                dict(stride=n - 1)):
        status, G = _gram(Yd, stride, n, ncol, check=False, bad=bad)
        assert status == -1 and np.all(np.isnan(G)), bad
        with pytest.raises(_lib.Emg3dAmdError, match="block_gram: "):
            _lib.check(status, 'emg3d_dev_block_gram')
    for bad in (dict(y=None), dict(t=None), dict(out=None), dict(n=0), dict(nout=0), dict(nin=2, nout=3), dict(nin=65, nout=3),
                dict(nin=0, nout=0), dict(stride=n - 1), dict(out_stride=n - 1)):
        status, out = _rotate(Yd, stride, n, 3, 2, Td, n + 2, check=False, bad=bad)
        assert status == -1 and np.all(np.isnan(out)), bad
        with pytest.raises(_lib.Emg3dAmdError, match="block_rotate: "):
            _lib.check(status, 'emg3d_dev_block_rotate')
    # out inside Y: on its first row, between two rows, and Y inside the rows of out
    from emg3d_amd._device import _stream
    import torch
    for offset in (0, stride + 3, 2 * stride + n - 1):
        assert L.emg3d_dev_block_rotate(n, 3, 2, _ptr(Yd), stride, _ptr(Td), _ptr(Yd, offset), stride, _stream()) == -1
    assert L.emg3d_dev_block_rotate(n, 3, 2, _ptr(Yd, stride), stride, _ptr(Td), _ptr(Yd), 2 * stride, _stream()) == -1
    torch.cuda.synchronize()
    assert np.array_equal(Yd.cpu().numpy(), Y, equal_nan=True)
    # behind the last row of Y is free: the good calls
    assert L.emg3d_dev_block_rotate(n, 3, 2, _ptr(Yd), stride, _ptr(Td), _ptr(Yd, 2 * stride + n), stride, _stream()) == 0
    G, _ = _gram(Yd, stride, n, ncol)
    assert not np.any(np.isnan(G))
    torch.cuda.synchronize()


# --------------------------------------------------------------- orthonormalisation on the gpu ---
@functools.lru_cache(maxsize=None)
def _orth_instance():
    hx, hy, hz = np.full(ORTH_SHAPE[0], 10.), np.full(ORTH_SHAPE[1], 30.), np.full(ORTH_SHAPE[2], 10.)
    grid = emg3d.TensorMesh([hx, hy, hz], (-95., -90., -50.))
    ones = np.ones(ORTH_SHAPE)
    model = emg3d.Model(grid, property_x=ones, property_y=2 * ones, property_z=3 * ones)
    return gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(ORTH_BLOCKS))
def test_orthonormalise_block(name):
    """Blocks of 3 x (19 x 6 x 7) rows and 12 columns with condition 1, 1e3, 1e6 and one with two equal columns: the rank
    is 12, 12, 12, 11; ``|Y - Q Q^T Y|_F / |Y|_F`` is within the span bound; ``max |Q^T Q - I|`` within 16 times that of
    ``numpy.linalg.qr`` (Householder) on the same block -- the NumPy model of the two passes stays within both
    (``test_the_orth_blocks_stay_within_the_cap_in_numpy``). The device route returns a device block with the same bits
    and leaves its input as it was; neither solves nor keeps anything."""
    import torch
    rec = _orth_instance()
    vectors, Y, sv, householder = _orth_block(name)
    Q, rank = rec.orthonormalise_block(vectors)
    assert rank == ORTH_BLOCKS[name][1] and Q.shape == (rank, 3) + ORTH_SHAPE and Q.dtype == np.float64
    Qf = Q.reshape(rank, -1).T                                   # (N, rank), rows ordered as those of Y
    orth = float(np.max(np.abs(Qf.T @ Qf - np.eye(rank))))
    span = float(np.linalg.norm(Y - Qf @ (Qf.T @ Y)) / np.linalg.norm(Y))
    record(f"orthonormalise_block, {name}: rank {rank}; max |Q^T Q - I| = {orth:.2e}, Householder QR {householder:.2e} (cap "
           f"{ORTH_FACTOR:.0f} x: ratio {orth / householder:.2f}); span {span:.2e} (bound {_span_bound(sv, rank):.2e})")
    assert span <= _span_bound(sv, rank)
    assert orth <= ORTH_FACTOR * householder
    B = rec.to_device(vectors)
    before = B.clone()
    Qd, rank_d = rec.orthonormalise_block(B)
    assert isinstance(Qd, torch.Tensor) and Qd.shape == (rank, 3, int(np.prod(ORTH_SHAPE))) and Qd.is_contiguous()
    assert rank_d == rank and torch.equal(B, before) and np.array_equal(rec.from_device(Qd), Q)
    assert np.array_equal(rec.orthonormalise_block(B, on_device=False)[0], Q)
    assert rec.n_solves == NONE and rec.kept_bytes == 0


@pytest.mark.gpu
def test_orthonormalise_a_block_of_zeros():
    """Rank 0, and an empty block of the form that was asked for: NumPy, or (0, n, n_cells) on the device."""
    import torch
    rec = _orth_instance()
    zeros = np.zeros((3, 3) + ORTH_SHAPE)
    Q, rank = rec.orthonormalise_block(zeros)
    assert rank == 0 and isinstance(Q, np.ndarray) and Q.shape == (0, 3) + ORTH_SHAPE
    for Qd, rank in (rec.orthonormalise_block(rec.to_device(zeros)), rec.orthonormalise_block(zeros, on_device=True)):
        assert rank == 0 and isinstance(Qd, torch.Tensor) and Qd.shape == (0, 3, int(np.prod(ORTH_SHAPE))) and Qd.device == _dev()
    Q, rank = rec.orthonormalise_block(rec.to_device(zeros), on_device=False)
    assert rank == 0 and isinstance(Q, np.ndarray) and Q.shape == (0, 3) + ORTH_SHAPE


# ----------------------------------------------------------------- the method on the gpu ---
CONFIGS = {'isotropic, device': dict(case='isotropic', mapping='Resistivity', keep='device'),
           'isotropic, host': dict(case='isotropic', mapping='Resistivity', keep='host'),
           'VTI, device': dict(case='VTI', mapping='LgConductivity', keep='device'),
           'VTI, host': dict(case='VTI', mapping='LgConductivity', keep='host'),
           'triaxial, device': dict(case='triaxial', mapping='LnResistivity', keep='device'),
           'VTI, computational grid': dict(case='VTI', mapping='Conductivity', keep='device', comp=True)}
JVEC_BLOCK = 1e-10                        # ``jvec_block`` vs ``jvec``, of the max-norm per pair (test_block_products)


def _weights(rec):
    """Non-trivial weights with a zero: the last receiver of the first pair carries none."""
    rng = np.random.default_rng(41)
    w = {p: rng.uniform(0.1, 2.0, len(RECS)) for p in rec.pairs}
    w[rec.pairs[0]][2] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def _reference(name, field_dtype='double'):
    """One configuration, once: the instance after ``forward()``, the weights, and the dense ``A* = W^1/2 J^`` (M, N) built
    row by row from ``jtvec`` of unit data in the ordering of ``stack_data`` -- ``jtvec(unit_i)`` is ``Re J_i``,
    ``jtvec(1j unit_i)`` is ``Im J_i`` --, every row flattened as ``reshape(-1)`` flattens the result of ``jtvec``; with
    its singular values, and the norms ``|J_i|_2`` of the complex rows."""
    spec = CONFIGS[name]
    grid, model = small_model(spec['case'], spec['mapping'])
    kw = dict(grids=_comp_grid()) if spec.get('comp') else {}
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, solver_opts=OPTS, tol_gradient=TOL, keep=spec['keep'],
                                         field_dtype=field_dtype, **kw)
    w = _weights(rec)
    nrec = len(RECS)
    rows = []
    for factor in (1.0, 1j):
        for pair in rec.pairs:
            for r in range(nrec):
                unit = np.zeros(nrec, dtype=complex)
                unit[r] = factor
                rows.append(rec.jtvec({pair: unit}).reshape(-1))
    J = np.stack(rows)
    M = len(J)
    root_w = np.tile(np.sqrt(np.concatenate([w[p] for p in rec.pairs])), 2)
    row_norm = np.sqrt(np.sum(J[:M // 2] ** 2, axis=1) + np.sum(J[M // 2:] ** 2, axis=1))
    A = root_w[:, None] * J
    return rec, w, A, np.linalg.svd(A, compute_uv=False), row_norm, root_w


def _error_of_b(rec, row_norm, root_w, columns):
    """``|E|_F`` for ``B = A* Q + E`` of ``columns`` columns. ``jvec_block`` gives every datum of a pair p within 1e-10 of
    the max-norm of the exact products of that pair (the bound ``test_block_products`` asserts against ``jvec``); for a
    unit column q that max-norm is at most ``max_{i in p} |J_i|_2`` (Cauchy-Schwarz), and the error of a complex datum
    bounds those of its real and imaginary rows. ``jtvec_block``, whose rows define ``A*``, is ``jtvec`` bit for bit."""
    nrec = len(RECS)
    per_pair = np.repeat([np.max(row_norm[i * nrec:(i + 1) * nrec]) for i in range(len(rec.pairs))], nrec)
    entry = JVEC_BLOCK * root_w * np.tile(per_pair, 2)
    return float(np.sqrt(columns * np.sum(entry ** 2)))


def _flat(V):
    return V.reshape(len(V), -1)


def _check_exact(name, field_dtype='double'):
    rec, w, A, s_ref, row_norm, root_w = _reference(name, field_dtype)
    M = len(A)
    solves = dict(rec.n_solves)
    U, s, V = rec.sensitivity_svd(M, weights=w)
    k = len(s)
    assert k == M - 2                                            # the two rows of the datum without a weight are zero
    assert U.shape == (M, k) and U.dtype == np.float64 and V.shape == (k,) + rec.jtvec({}).shape and V.dtype == np.float64
    assert np.all(np.diff(s) <= 0) and np.all(s > 0)
    Vf = _flat(V)
    err_b = _error_of_b(rec, row_norm, root_w, k)
    orth_v = float(np.linalg.norm(Vf @ Vf.T - np.eye(k), 2))     # (k = l': V = Q W with W orthogonal)
    orth_u = float(np.max(np.abs(U.T @ U - np.eye(k))))
    ds = float(np.max(np.abs(s - s_ref[:k])))
    da = float(np.linalg.norm((U * s) @ Vf - A))
    cap = err_b + s_ref[0] * orth_v
    zero = np.flatnonzero(root_w == 0)
    dz = float(np.max(np.abs((U * s)[zero])))
    record(f"sensitivity_svd exact, {name}, {field_dtype}: k = {k} of M = {M}; s_1 = {s_ref[0]:.3e}, s_k / s_1 = "
           f"{s_ref[k - 1] / s_ref[0]:.2e}; max |s - s*| / |E|_F = {ds / err_b:.2e}; |U s V^T - A*|_F / (|E|_F + |A*| |Q^T Q - I|) "
           f"= {da / cap:.2e}; |Q^T Q - I|_2 = {orth_v:.2e}, max |U^T U - I| = {orth_u:.2e}; rows without a weight "
           f"{dz / cap:.2e} of the bound")
    assert len(zero) == 2
    assert ds <= err_b                                           # Weyl
    assert da <= cap
    assert dz <= cap                                             # (a row of the difference to A*, whose row is zero)
    assert orth_u <= 100 * k * EPS                               # LAPACK's U: O(k eps)
    top = np.argmax(np.abs(U), axis=0)
    assert np.all(U[top, np.arange(k)] > 0)                      # the sign convention
    assert rec.n_solves == solves and solves['jvec'] == solves['jtvec'] == 0
    return rec, w, (U, s, V)


@pytest.mark.gpu
@pytest.mark.parametrize('name', [c for c in CONFIGS if 'grid' not in c])
def test_exact_case_against_the_dense_svd(name):
    """``rank = M``: l = M and the sketch spans every row of ``A* = W^1/2 J^``. Against ``numpy.linalg.svd`` of the dense
    matrix from ``jtvec`` of unit data, with weights that include a zero: ``|s - s*| <= |E|_F`` (Weyl), ``|U diag(s) V^T -
    A*|_F <= |E|_F + |A*|_2 |Q^T Q - I|_2``, E as ``_error_of_b`` derives it; the datum without a weight gives two zero
    rows of ``U diag(s)`` and k = M - 2; the sign convention; nothing is solved."""
    _check_exact(name)


@pytest.mark.gpu
def test_other_computational_grids():
    """``grids=_comp_grid()``: the exact case holds against the ``jtvec`` rows of that object, while ``data_gram()`` on the
    same object still refuses."""
    rec, w, _ = _check_exact('VTI, computational grid')
    with pytest.raises(NotImplementedError, match="is not the model grid"):
        rec.data_gram()


def _hmt(sv, k, p, q):
    """Halko, Martinsson, Tropp, Corollary 10.10: the expectation of ``|A - Q Q^T A|_2`` after q power iterations."""
    tail = sv[k:]
    e = 2 * q + 1
    return float(((1 + np.sqrt(k / (p - 1))) * tail[0] ** e + np.e * np.sqrt(k + p) / p * np.sqrt(np.sum(tail ** (2 * e)))) ** (1 / e))


def _restated(A, k, p, q, seed):
    """The algorithm in NumPy on the dense matrix with the same ``Omega``: the spectral error of its rank-k result."""
    M = len(A)
    omega = np.random.default_rng(seed).standard_normal((M, min(k + p, M)))
    Q, _ = np.linalg.qr(A.T @ omega)
    for _ in range(q):
        Q, _ = np.linalg.qr(A.T @ (A @ Q))
    U, s, Wt = np.linalg.svd(A @ Q, full_matrices=False)
    return float(np.linalg.norm(A - (U[:, :k] * s[:k]) @ (Wt[:k] @ Q.T), 2)), s[:k]


TRUNCATED_SEED = 0
# Against the NumPy restatement with the same Omega the 1e-10 of ``jvec_block`` is far too wide a yardstick: both routes
# compute the singular values of the same ``A* Q`` and differ by rounding alone. Every step of the method -- the
# combination of ``jtvec``, the sums of a Gram matrix and its rotation (twice per orthonormalisation), the dots of
# ``jvec`` -- is a sum of at most n_edges terms, each within ``(n + 16) eps`` of the sum of the magnitudes of its terms, the
# project's bound for a sum; relative to ``s_1 = |A*|_2`` that is ``(n_edges + 16) eps`` per step to first order. Eight
# steps for q = 0 (jtvec, 2 x (gram, rotate), jvec, the host SVD, the restatement's own rounding); a power iteration
# converges towards the leading subspace and does not add to the error of the LEADING values, so the same count holds
# for q = 2. About 4e-12 s_1 on these grids; a relative error of 1e-11 in the orthonormalisation or in the final
# rotation does not pass.
ROUNDING_STEPS = 8


@pytest.mark.gpu
@pytest.mark.parametrize('q', [0, 2])
@pytest.mark.parametrize('name', ['isotropic, device', 'VTI, device', 'VTI, host', 'triaxial, device'])
def test_truncated_case(name, q):
    """``rank = 4``, ``oversample = 2``: ``s_j <= s*_j + |E|_F`` for every j (the singular values of ``A Q`` never exceed
    those of A) and ``|A* - U diag(s) V^T|_2 <= 2 x`` the expectation bound of Halko, Martinsson and Tropp at k = 4, p = 2
    and q. That is a cap, not a measurement: the seed is one for which the NumPy restatement of the algorithm on the
    dense ``A*`` with the same ``Omega`` stays under the expectation bound itself, asserted here before the result is
    looked at (on the CPU the restatement was run on a dense stand-in with a spectrum over five decades; with seed 0 it
    stayed at 0.15 and 0.69 of the bound, and on this survey's ``A*`` at 0.16 and 0.69). Last, against that restatement:
    ``|s - s_numpy| <= 8 (n_edges + 16) eps s_1`` (``ROUNDING_STEPS``), the yardstick that bites on rounding-sized errors."""
    rec, w, A, s_ref, row_norm, root_w = _reference(name)
    k, p = 4, 2
    bound = _hmt(s_ref, k, p, q)
    restated, s_np = _restated(A, k, p, q, TRUNCATED_SEED)
    assert restated <= bound                                     # the seed: a condition on the inputs
    U, s, V = rec.sensitivity_svd(k, weights=w, oversample=p, power_iterations=q, seed=TRUNCATED_SEED)
    assert len(s) == k and U.shape == (len(A), k) and len(V) == k
    err_b = _error_of_b(rec, row_norm, root_w, k + p)
    err = float(np.linalg.norm(A - (U * s) @ _flat(V), 2))
    over = float(np.max((s - s_ref[:k]) / err_b))
    record(f"sensitivity_svd truncated, {name}, q = {q}: |A* - U s V^T|_2 = {err:.3e}, NumPy with the same Omega {restated:.3e}, "
           f"expectation bound {bound:.3e}, s*_5 = {s_ref[k]:.3e}; max (s - s*) / |E|_F = {over:.2e}; max |s - s_numpy| / s_1 = "
           f"{float(np.max(np.abs(s - s_np)) / s_ref[0]):.2e}")
    assert np.all(s <= s_ref[:k] + err_b)
    assert err <= 2 * bound
    # the same Omega, the same algorithm: only rounding separates the two sets of singular values
    n_terms = max(rec._grid_of(p).n_edges for p in rec.pairs)
    assert np.max(np.abs(s - s_np)) <= ROUNDING_STEPS * (n_terms + 16) * EPS * s_ref[0]


@pytest.mark.gpu
def test_conventions():
    """The same arguments twice: the same bits. ``on_device=True``: a float64 block (k, n, n_cells) on the device of the
    fields, equal to the host result. The sign convention. Another seed: another sketch. ``columns_per_pass`` regroups
    the columns of a pass: the singular values agree within twice ``|E|_F``. Nothing is solved."""
    import torch
    rec, w, A, s_ref, row_norm, root_w = _reference('VTI, device')
    solves = dict(rec.n_solves)
    U, s, V = rec.sensitivity_svd(4, weights=w, oversample=2)
    U2, s2, V2 = rec.sensitivity_svd(4, weights=w, oversample=2)
    assert np.array_equal(U, U2) and np.array_equal(s, s2) and np.array_equal(V, V2)
    Ud, sd, Vd = rec.sensitivity_svd(4, weights=w, oversample=2, on_device=True)
    assert isinstance(Vd, torch.Tensor) and Vd.dtype == torch.float64 and Vd.shape == (4, 2, rec.model.grid.n_cells)
    assert Vd.device == _dev() and Vd.is_contiguous()
    assert np.array_equal(rec.from_device(Vd), V) and np.array_equal(Ud, U) and np.array_equal(sd, s)
    top = np.argmax(np.abs(U), axis=0)
    assert np.all(U[top, np.arange(4)] > 0)
    U3, s3, V3 = rec.sensitivity_svd(4, weights=w, oversample=2, columns_per_pass=2)
    assert np.max(np.abs(s3 - s)) <= _error_of_b(rec, row_norm, root_w, 6) * 2
    U4, s4, V4 = rec.sensitivity_svd(4, weights=w, oversample=2, seed=7)
    assert not np.array_equal(s4, s)
    assert rec.n_solves == solves and solves['jvec'] == solves['jtvec'] == 0


@pytest.mark.gpu
def test_single_stored_fields():
    """``field_dtype='single'`` against ``'double'``: the singular values within 1e-6 of ``s_1`` -- every kept value
    carries a relative error of at most 2^-24 = 6e-8 (the class docstring), a product of two of them 1.2e-7 of the sum of
    the magnitudes of its terms."""
    rec, w, A, s_ref, _, _ = _reference('VTI, device')
    single, *_ = _reference('VTI, device', 'single')
    M = len(A)
    _, s, _ = rec.sensitivity_svd(M, weights=w)
    _, s1, _ = single.sensitivity_svd(M, weights=w)
    assert len(s) == len(s1) == M - 2
    worst = float(np.max(np.abs(s - s1)) / s[0])
    record(f"sensitivity_svd single vs double: max |s - s'| / s_1 = {worst:.2e} (bound 1e-6)")
    assert worst <= 1e-6
