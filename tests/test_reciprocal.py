"""Solve-free sensitivity products: the four kernels of ``csrc/reciprocal.h`` (``emg3d_dev_edge_weights``,
``emg3d_dev_sensitivity_dots``, ``emg3d_dev_sensitivity_combine``, ``emg3d_dev_edges_to_cells``) against NumPy written
out in this file, and ``gradient.ReciprocalSensitivity`` against ``gradient.Sensitivity``.

Inputs, the small survey and the recorder come from ``test_sensitivity``; figures that the GPU tests observe are
printed and, with ``EMG3D_AMD_PARITY_FILE`` set, appended to that file (``profiles/reciprocal_parity.txt`` is such a
run).
"""
import functools
import gc

import numpy as np
import pytest

import emg3d_amd as emg3d
from emg3d_amd import _lib, gradient, parallel
from helpers import widths
from test_sensitivity import (ADJOINT_CASES, EPS, FREQS, MU_0, OPTS, RECS, SRCS, TOL, _fd_inputs, _maxdiff, _random_data,
                              _stretched, cells_to_edges, record, small_model)

SYMBOLS = ('emg3d_dev_edge_weights', 'emg3d_sensitivity_dots_ws_len', 'emg3d_dev_sensitivity_dots',
           'emg3d_dev_sensitivity_combine', 'emg3d_dev_edges_to_cells')


# ----------------------------------------------------------------------- not gpu tests ---
def test_public_name_and_declared_symbols():
    assert 'ReciprocalSensitivity' in gradient.__all__
    header = open(_lib.HEADER).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name) and name + '(' in header


def test_construction_needs_no_device():
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    assert rec.n_solves == {'forward': 0, 'receiver': 0, 'jvec': 0, 'jtvec': 0}
    assert rec.kept_bytes == 0 and rec.keep == 'device'
    text = repr(rec)
    assert "2 pairs" in text and "3 receiver fields" in text and "keep='device'" in text and "0 B" in text
    assert "keep='host'" in repr(gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, keep='host'))
    for keep in (False, None):
        with pytest.raises(ValueError, match="nothing to be solve-free from"):
            gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, keep=keep)
    with pytest.raises(ValueError, match="`keep` must be"):
        gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, keep='disk')


def _comp_grid(n=6):
    cx, cz = widths(n, 3, 35., 1.25), widths(n, 3, 28., 1.25)
    return emg3d.TensorMesh([cx, cx, cz], (-cx.sum() / 2, -cx.sum() / 2, -cz[:n].sum()))


def test_one_computational_grid_per_frequency():
    grid, model = small_model()
    freqs = {'lo': 1.0, 'hi': 2.5}
    one, same, other = _comp_grid(), _comp_grid(), _comp_grid(8)
    ok = {('a', 'lo'): one, ('b', 'lo'): same, ('a', 'hi'): other, ('b', 'hi'): other}     # `==` and `is`
    rec = gradient.ReciprocalSensitivity(model, SRCS, freqs, RECS, grids=ok)
    assert rec.grids[('a', 'lo')] is rec.grids[('b', 'lo')]
    gradient.ReciprocalSensitivity(model, SRCS, freqs, RECS, grids=one)
    gradient.ReciprocalSensitivity(model, SRCS, freqs, RECS, grids={('a', 'hi'): grid})      # the model's grid: as none
    for bad in ({('a', 'lo'): one, ('b', 'lo'): one, ('a', 'hi'): one, ('b', 'hi'): other},
                {('b', 'hi'): other}):
        with pytest.raises(ValueError, match="frequency 'hi' must share one computational grid"):
            gradient.ReciprocalSensitivity(model, SRCS, freqs, RECS, grids=bad)
    gradient.Sensitivity(model, SRCS, freqs, RECS, grids=bad)                                 # (fine there)


def test_more_than_one_rank_is_refused(monkeypatch):
    grid, model = small_model()
    monkeypatch.setattr(parallel, 'rank_and_world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="one process"):
        gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)


@pytest.mark.parametrize('case, n', [('isotropic', 1), ('HTI', 2), ('VTI', 2), ('triaxial', 3)])
def test_vectors_are_validated_as_by_sensitivity(case, n):
    """The same exceptions with the same messages as ``Sensitivity``, before any GPU work."""
    grid, model = small_model(case)
    shape = tuple(grid.shape_cells)
    lin = gradient.Sensitivity(model, SRCS, FREQS, RECS)
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)

    def message(call):
        with pytest.raises(ValueError) as err:
            call()
        return str(err.value)
    for bad in ((n + 1,) + shape, shape[:2]) + (() if n == 1 else (shape,)):
        assert message(lambda: rec.jvec(np.zeros(bad))) == message(lambda: lin.jvec(np.zeros(bad)))
    cv = np.zeros((n,) + shape, dtype=complex)
    assert "must be real" in message(lambda: rec.jvec(cv)) == message(lambda: lin.jvec(cv))
    y = {('a', 'f'): np.zeros(len(RECS) + 1, dtype=complex)}
    assert "one value per receiver" in message(lambda: rec.jtvec(y)) == message(lambda: lin.jtvec(y))
    assert rec.n_solves == {'forward': 0, 'receiver': 0, 'jvec': 0, 'jtvec': 0}


def test_epsilon_r_and_mu_r_are_refused():
    grid, model = small_model()
    ones = np.ones(grid.shape_cells)
    for kw, name in (({'epsilon_r': 2 * ones}, 'el. permittivity'), ({'mu_r': 2 * ones}, 'magn. permeability')):
        with pytest.raises(NotImplementedError, match=f"Gradient not implemented for {name}"):
            gradient.ReciprocalSensitivity(emg3d.Model(grid, property_x=ones, **kw), SRCS, FREQS, RECS)
    gradient.ReciprocalSensitivity(emg3d.Model(grid, property_x=ones, epsilon_r=ones, mu_r=ones), SRCS, FREQS, RECS)


def test_no_cpu_fallback_without_gpu():
    if _lib.lib().emg3d_device_count() > 0:
        pytest.skip("GPU present")
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.jvec(np.ones(grid.shape_cells))
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.jtvec({('a', 'f'): np.ones(3, dtype=complex)})
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.synthetic
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.forward()


# ------------------------------------------------------------------ kernels on the gpu ---
def _dev():
    import torch
    return torch.device('cuda', torch.cuda.current_device())


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _stack(rng, rows, n, is_complex):
    """(rows, stride) with stride > n: random fields, and NaN between them, which must never be read."""
    stride = n + 3 + rows
    a = np.full((rows, stride), np.nan, dtype=complex if is_complex else float)
    a[:, :n] = rng.standard_normal((rows, n)) + (1j * rng.standard_normal((rows, n)) if is_complex else 0)
    return a, stride


def _dots(E, es, X, xs, n, w, scale, is_complex):
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    ns, nr = len(E), len(X)
    ws_len = L.emg3d_sensitivity_dots_ws_len(ns, nr, n)
    ws = torch.full((ws_len,), float('nan'), dtype=torch.float64, device=_dev())
    out = torch.full((ns * nr,), float('nan'), dtype=E.dtype, device=_dev())
    _lib.check(L.emg3d_dev_sensitivity_dots(n, int(is_complex), _ptr(E), es, ns, _ptr(X), xs, nr, _ptr(w),
                                            complex(scale).real, complex(scale).imag, _ptr(out), _ptr(ws), ws_len, _stream()),
               'emg3d_dev_sensitivity_dots')
    return out.cpu().numpy().reshape(ns, nr)


def _combine(E, es, X, xs, n, coef, is_complex):
    import torch
    from emg3d_amd._device import _ptr, _stream
    t = torch.full((n,), float('nan'), dtype=E.dtype, device=_dev())          # every entry must be WRITTEN
    _lib.check(_lib.lib().emg3d_dev_sensitivity_combine(n, int(is_complex), _ptr(E), es, len(E), _ptr(X), xs, len(X),
                                                        _ptr(coef), _ptr(t), _stream()), 'emg3d_dev_sensitivity_combine')
    return t.cpu().numpy()


SIZES = [1, 257, 70001]        # one workgroup of the dots kernel covers 8192 entries: 70 001 are nine of them
TILES = [(1, 1), (3, 5), (9, 2), (4, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('ns, nr', TILES)
@pytest.mark.parametrize('n', SIZES)
def test_dots_vs_numpy(n, ns, nr, is_complex):
    """``|got - want| <= (n + 16) eps |scale| sum_k |w_k| |e_s[k]| |x_r[k]|`` per entry: the worst case of ANY order of
    summation plus the few roundings of a term. The largest size is summed a second time: the same bits."""
    rng = np.random.default_rng(n + 10 * ns + nr + is_complex)
    (E, es), (X, xs) = _stack(rng, ns, n, is_complex), _stack(rng, nr, n, is_complex)
    w = rng.standard_normal(n)
    scale = 0.3 - 1.7j if is_complex else 0.7
    Ed, Xd, wd = _up(E), _up(X), _up(w)
    got = _dots(Ed, es, Xd, xs, n, wd, scale, is_complex)
    want = scale * np.einsum('k,sk,rk->sr', w, E[:, :n], X[:, :n])
    bound = (n + 16) * EPS * abs(scale) * np.einsum('k,sk,rk->sr', np.abs(w), np.abs(E[:, :n]), np.abs(X[:, :n]))
    assert got.dtype == E.dtype and not np.any(np.isnan(got))
    worst = float(np.max(np.abs(got - want) / bound))
    record(f"dots n={n} ns={ns} nr={nr} complex={is_complex}: max |diff| / bound = {worst:.2e} (bound (n + 16) eps)")
    assert np.all(np.abs(got - want) <= bound)
    if n == SIZES[-1]:
        assert np.array_equal(got, _dots(Ed, es, Xd, xs, n, wd, scale, is_complex))


@pytest.mark.gpu
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('ns, nr', TILES + [(2, 11)])
@pytest.mark.parametrize('n', SIZES)
def test_combine_vs_numpy(n, ns, nr, is_complex):
    """``|got - want| <= (ns nr + 16) eps sum_{s,r} |e_s[k]| |coef_{s,r}| |x_r[k]|`` per entry; (2, 11): receivers
    beyond the eight whose values a thread keeps in registers. Twice: the same bits."""
    rng = np.random.default_rng(3 * n + 10 * ns + nr + is_complex)
    (E, es), (X, xs) = _stack(rng, ns, n, is_complex), _stack(rng, nr, n, is_complex)
    coef = rng.standard_normal((ns, nr)) + (1j * rng.standard_normal((ns, nr)) if is_complex else 0)
    Ed, Xd, cd = _up(E), _up(X), _up(coef)
    got = _combine(Ed, es, Xd, xs, n, cd, is_complex)
    want = np.sum(E[:, :n] * (coef @ X[:, :n]), axis=0)
    bound = (ns * nr + 16) * EPS * np.sum(np.abs(E[:, :n]) * (np.abs(coef) @ np.abs(X[:, :n])), axis=0)
    assert got.dtype == E.dtype and not np.any(np.isnan(got))
    worst = float(np.max(np.abs(got - want) / bound))
    record(f"combine n={n} ns={ns} nr={nr} complex={is_complex}: max |diff| / bound = {worst:.2e} "
           f"(bound (ns nr + 16) eps)")
    assert np.all(np.abs(got - want) <= bound)
    assert np.array_equal(got, _combine(Ed, es, Xd, xs, n, cd, is_complex))


def _flat(parts):
    return np.concatenate([c.ravel('F') for c in parts])


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(67, 5, 9), (12, 10, 8)])
@pytest.mark.parametrize('alias', [True, False])
def test_edge_weights_vs_numpy(shape, alias):
    """Against ``cells_to_edges(vol * v)`` within ``4 eps 1/4 sum |vol v|`` over the edge's cells, a bound on the
    magnitude of the factors (three additions and the products, fused here, rounded separately by NumPy)."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    grid = _stretched(*shape)
    rng = np.random.default_rng(sum(shape) + alias)
    v3 = rng.standard_normal((3,) + shape)
    if alias:
        v3[1:] = v3[0]
    vol = grid.cell_volumes.reshape(shape, order='F')
    vd = [_up(c.ravel('F')) for c in v3]
    if alias:
        vd = [vd[0]] * 3
    o1, o2 = grid.n_edges_x, grid.n_edges_x + grid.n_edges_y
    w = torch.full((grid.n_edges,), float('nan'), dtype=torch.float64, device=_dev())       # every edge is WRITTEN
    _lib.check(_lib.lib().emg3d_dev_edge_weights(*shape, _ptr(_up(grid.cell_volumes.astype(np.float64))), _ptr(vd[0]),
                                                 _ptr(vd[1]), _ptr(vd[2]), _ptr(w), _ptr(w, o1), _ptr(w, o2), _stream()),
               'emg3d_dev_edge_weights')
    got = w.cpu().numpy()
    want, mag = _flat(cells_to_edges(vol[None] * v3)), _flat(cells_to_edges(np.abs(vol[None] * v3)))
    assert not np.any(np.isnan(got))
    worst = float(np.max(np.abs(got - want) / (4 * EPS * mag)))
    record(f"edge_weights {shape} alias={alias}: max |diff| / bound = {worst:.3f} (bound 4 eps)")
    assert np.all(np.abs(got - want) <= 4 * EPS * mag)


def _edges_to_cells_numpy(grid, t, smu0, g0):
    """g0 + volume / 4 * sum real(s mu0 t) over the four x-, y-, z-edges of a cell, z outer, then y, then x."""
    nx, ny, nz = grid.shape_cells
    vol = grid.cell_volumes.reshape(grid.shape_cells, order='F')
    o1, o2 = grid.n_edges_x, grid.n_edges_x + grid.n_edges_y
    r = np.real(smu0 * t)
    rx, ry, rz = (r[:o1].reshape((nx, ny + 1, nz + 1), order='F'), r[o1:o2].reshape((nx + 1, ny, nz + 1), order='F'),
                  r[o2:].reshape((nx + 1, ny + 1, nz), order='F'))
    g = g0.copy()
    for d2 in (0, 1):
        for d1 in (0, 1):
            g[0] += vol * rx[:, d1:ny + d1, d2:nz + d2] / 4
            g[1] += vol * ry[d1:nx + d1, :, d2:nz + d2] / 4
            g[2] += vol * rz[d1:nx + d1, d2:ny + d2, :] / 4
    return g


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(67, 5, 9), (12, 10, 8)])
@pytest.mark.parametrize('is_complex', [True, False])
def test_edges_to_cells_vs_numpy_and_gradient_accumulate(shape, is_complex):
    """With a non-zero starting g, against the NumPy restatement and against ``emg3d_dev_gradient_accumulate(e, b)``
    for ``t = b e``, both within ``16 eps (|g0| + vol / 4 |s mu0| sum |t|)``."""
    from emg3d_amd._device import _ptr, _stream
    grid = _stretched(*shape)
    rng = np.random.default_rng(sum(shape) + 5 * is_complex)
    n, nc = grid.n_edges, grid.n_cells
    e, b = (rng.standard_normal(n) + (1j * rng.standard_normal(n) if is_complex else 0) for _ in range(2))
    t = b * e
    smu0 = 2j * np.pi * 0.7 * MU_0 if is_complex else 0.7 * MU_0
    g0 = rng.standard_normal((3,) + shape) * 1e-3
    vol = _up(grid.cell_volumes.astype(np.float64))
    o1, o2 = grid.n_edges_x, grid.n_edges_x + grid.n_edges_y
    td, ed, bd = _up(t), _up(e), _up(b)
    g, ga = _up(_flat(g0)), _up(_flat(g0))
    s = complex(smu0)
    _lib.check(_lib.lib().emg3d_dev_edges_to_cells(*shape, int(is_complex), _ptr(td), _ptr(td, o1), _ptr(td, o2), s.real,
                                                   s.imag, _ptr(vol), _ptr(g), _ptr(g, nc), _ptr(g, 2 * nc), _stream()),
               'emg3d_dev_edges_to_cells')
    _lib.check(_lib.lib().emg3d_dev_gradient_accumulate(
        *shape, int(is_complex), _ptr(ed), _ptr(ed, o1), _ptr(ed, o2), _ptr(bd), _ptr(bd, o1), _ptr(bd, o2), s.real, s.imag,
        _ptr(vol), _ptr(ga), _ptr(ga, nc), _ptr(ga, 2 * nc), _stream()), 'emg3d_dev_gradient_accumulate')
    got, acc = g.cpu().numpy(), ga.cpu().numpy()
    want = _flat(_edges_to_cells_numpy(grid, t, smu0, g0))
    bound = 16 * EPS * _flat(_edges_to_cells_numpy(grid, np.abs(t), abs(smu0), np.abs(g0)))
    worst = [float(np.max(np.abs(got - ref) / bound)) for ref in (want, acc)]
    record(f"edges_to_cells {shape} complex={is_complex}: max |diff| / bound = {worst[0]:.3f} vs NumPy, {worst[1]:.3f} vs "
           f"gradient_accumulate (bound 16 eps)")
    assert np.all(np.abs(got - want) <= bound) and np.all(np.abs(got - acc) <= bound)


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    a = torch.zeros(64, dtype=torch.complex128, device=_dev())
    d = torch.zeros(64, dtype=torch.float64, device=_dev())
    p, q = _ptr(a), _ptr(d)
    calls = {
        'edge_weights': [lambda: L.emg3d_dev_edge_weights(2, 2, 2, None, q, q, q, q, q, q, _stream()),
                         lambda: L.emg3d_dev_edge_weights(2, 2, 2, q, q, q, q, q, None, q, _stream()),
                         lambda: L.emg3d_dev_edge_weights(0, 2, 2, q, q, q, q, q, q, q, _stream())],
        'sensitivity_dots': [lambda: L.emg3d_dev_sensitivity_dots(4, 1, None, 4, 1, p, 4, 1, q, 1., 0., p, q, 64, _stream()),
                             lambda: L.emg3d_dev_sensitivity_dots(4, 1, p, 4, 1, p, 4, 1, q, 1., 0., p, None, 64, _stream()),
                             lambda: L.emg3d_dev_sensitivity_dots(4, 1, p, 4, 0, p, 4, 1, q, 1., 0., p, q, 64, _stream()),
                             lambda: L.emg3d_dev_sensitivity_dots(4, 1, p, 4, 1, p, 4, 1, q, 1., 0., p, q, 1, _stream()),
                             lambda: L.emg3d_dev_sensitivity_dots(4, 1, p, 3, 2, p, 4, 1, q, 1., 0., p, q, 64, _stream())],
        'sensitivity_combine': [lambda: L.emg3d_dev_sensitivity_combine(4, 1, p, 4, 1, None, 4, 1, p, p, _stream()),
                                lambda: L.emg3d_dev_sensitivity_combine(4, 1, p, 4, 1, p, 4, 1, p, None, _stream()),
                                lambda: L.emg3d_dev_sensitivity_combine(4, 1, p, 4, 0, p, 4, 1, p, p, _stream()),
                                lambda: L.emg3d_dev_sensitivity_combine(0, 1, p, 4, 1, p, 4, 1, p, p, _stream())],
        'edges_to_cells': [lambda: L.emg3d_dev_edges_to_cells(2, 2, 2, 1, None, p, p, 0., 1., q, q, q, q, _stream()),
                           lambda: L.emg3d_dev_edges_to_cells(2, 2, 2, 1, p, p, p, 0., 1., q, q, q, None, _stream()),
                           lambda: L.emg3d_dev_edges_to_cells(2, 0, 2, 1, p, p, p, 0., 1., q, q, q, q, _stream())],
    }
    for name, bad in calls.items():
        for call in bad:
            with pytest.raises(_lib.Emg3dAmdError, match=f"{name}: "):
                _lib.check(call(), 'emg3d_dev_' + name)
    assert L.emg3d_sensitivity_dots_ws_len(0, 1, 4) == 0
    assert L.emg3d_sensitivity_dots_ws_len(3, 5, 70001) == 2 * 15 * 9


# ----------------------------------------------------------------- products on the gpu ---
@functools.lru_cache(maxsize=None)
def _both(name):
    """One entry of ADJOINT_CASES through both classes, once: (grid, model, Sensitivity, ReciprocalSensitivity, v, y,
    and the four products). Some data are NaN."""
    spec = ADJOINT_CASES[name]
    grid, model = small_model(spec['case'], spec['mapping'])
    kw = dict(solver_opts=OPTS, tol_gradient=TOL, magnetic=spec.get('magnetic'))
    if spec.get('comp'):
        kw['grids'] = _comp_grid()             # the computational grid of test_jvec_and_jtvec_are_adjoint
    lin = gradient.Sensitivity(model, SRCS, FREQS, RECS, **kw)
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, **kw)
    rng = np.random.default_rng(17)
    v = rng.standard_normal((gradient._NCOMP[spec['case']],) + tuple(grid.shape_cells))
    y = _random_data(rng, lin.pairs, len(RECS))
    y[('a', 'f')][1] = np.nan
    y[('b', 'f')][0] = np.nan
    out = dict(jv_lin=lin.jvec(v), jt_lin=lin.jtvec(y), jv_rec=rec.jvec(v), jt_rec=rec.jtvec(y))
    return grid, model, lin, rec, v, y, out


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(ADJOINT_CASES))
def test_products_equal_the_solving_path(name):
    """``jvec`` and ``jtvec`` of both classes for the same v and y (some NaN), all solves at 1e-10: max-norm relative
    difference <= 1e-6, the criterion of test_jvec_and_jtvec_are_adjoint for these operators at this tolerance. Pins
    the factor of jvec and every conjugation. The forward responses are the same bits."""
    grid, model, lin, rec, v, y, out = _both(name)
    dv, dt = _maxdiff(out['jv_rec'], out['jv_lin']), _maxdiff(out['jt_rec'], out['jt_lin'])
    record(f"reciprocal vs solving path, {name}: jvec {dv:.2e}, jtvec {dt:.2e} (bound 1e-6)")
    assert list(out['jv_rec']) == lin.pairs and out['jt_rec'].shape == out['jt_lin'].shape
    assert all(out['jv_rec'][p].shape == (len(RECS),) and np.iscomplexobj(out['jv_rec'][p]) for p in lin.pairs)
    assert all(np.array_equal(rec.synthetic[p], lin.synthetic[p]) for p in lin.pairs)
    assert rec.n_solves == {'forward': 2, 'receiver': 3, 'jvec': 0, 'jtvec': 0}
    assert set(rec.info) == set(lin.pairs) | {('receiver', r, 'f') for r in range(3)}
    assert dv <= 1e-6 and dt <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['isotropic', 'triaxial'])
def test_products_are_adjoint_to_rounding(case):
    """No solve separates the two products, so with the mapping 'Conductivity'
    ``|sum v jtvec(y) - Re sum conj(y) jvec(v)| <= (n_edges + 64) eps S``,
    ``S = |s mu0| sum_{s,r} |y_{s,r}| sum_k w_k(|v|) |e_s[k]| |x_r[k]|`` from the kept fields: the bound of any order of
    summation, which cancellation cannot break."""
    grid, model = small_model(case, 'Conductivity')
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, solver_opts=OPTS, tol_gradient=TOL)
    rng = np.random.default_rng(53)
    v = rng.standard_normal((gradient._NCOMP[case],) + tuple(grid.shape_cells))
    y = _random_data(rng, rec.pairs, len(RECS))
    y[('b', 'f')][2] = np.nan
    jv, jt = rec.jvec(v), rec.jtvec(y)
    lhs = float(np.sum(v.reshape(jt.shape) * jt))
    rhs = float(sum(np.nansum(np.conj(y[p]) * jv[p]).real for p in rec.pairs))
    E, X = (t.cpu().numpy() for t in rec._stacks['f'])
    vol = grid.cell_volumes.reshape(grid.shape_cells, order='F')
    w = _flat(cells_to_edges(vol[None] * gradient.expand_vector(model, np.abs(v))))
    ay = np.abs(np.nan_to_num(np.stack([y[p] for p in rec.pairs])))
    S = 2 * np.pi * FREQS['f'] * MU_0 * float(np.sum(ay * np.einsum('k,sk,rk->sr', w, np.abs(E), np.abs(X))))
    bound = (grid.n_edges + 64) * EPS * S
    record(f"adjoint to rounding, {case}: sum(v jtvec(y)) {lhs:.15e}  Re sum conj(y) jvec(v) {rhs:.15e}  |diff| "
           f"{abs(lhs - rhs):.2e} = {abs(lhs - rhs) / bound:.2e} x bound ((n_edges + 64) eps S = {bound:.2e}); relative "
           f"{abs(lhs - rhs) / abs(lhs):.2e}")
    assert abs(lhs - rhs) <= bound


@pytest.mark.gpu
def test_no_product_solves_anything():
    grid, model = small_model('VTI')
    freqs = {'f1': 1.0, 'f2': 2.5}
    rec = gradient.ReciprocalSensitivity(model, SRCS, freqs, RECS, solver_opts=OPTS, tol_gradient=TOL)
    rng = np.random.default_rng(59)
    v = rng.standard_normal((2,) + tuple(grid.shape_cells))
    y = _random_data(rng, rec.pairs, len(RECS))
    assert rec.forward() is rec
    counts = {'forward': 4, 'receiver': 6, 'jvec': 0, 'jtvec': 0}
    assert rec.n_solves == counts and rec.kept_bytes == (4 + 6) * grid.n_edges * 16
    assert "6 receiver fields" in repr(rec) and f"{rec.kept_bytes:,} B" in repr(rec)
    jv = [rec.jvec(v) for _ in range(3)]
    jt = [rec.jtvec(y) for _ in range(3)]
    assert rec.forward() is rec and rec.n_solves == counts
    assert list(jv[0]) == rec.pairs and jt[0].shape == (2,) + tuple(grid.shape_cells)
    same = all(np.array_equal(jv[0][p], j[p]) for j in jv for p in rec.pairs) and all(np.array_equal(jt[0], j) for j in jt)
    record(f"three jvec and three jtvec after forward(): n_solves {rec.n_solves}; bit-identical: {same}")
    assert same


@pytest.mark.gpu
def test_misfit_and_gradient_vs_sensitivity():
    grid, model, obs, wts = _fd_inputs()
    obs[('a', 'f')][1] = np.nan
    lin = gradient.Sensitivity(model, SRCS, FREQS, RECS, solver_opts=OPTS, tol_gradient=TOL)
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, solver_opts=OPTS, tol_gradient=TOL)
    m0, g0 = lin.misfit_and_gradient(obs, wts)
    m1, g1 = rec.misfit_and_gradient(obs, wts)
    record(f"misfit_and_gradient, reciprocal vs solving path: misfit rel {abs(m1 - m0) / m0:.2e} (bound 1e-12), gradient "
           f"{_maxdiff(g1, g0):.2e} (bound 1e-6)")
    assert abs(m1 - m0) <= 1e-12 * m0
    assert g1.shape == g0.shape and _maxdiff(g1, g0) <= 1e-6
    assert rec.n_solves == {'forward': 2, 'receiver': 3, 'jvec': 0, 'jtvec': 0}


@pytest.mark.gpu
def test_host_kept_fields_batched_receiver_solves_and_release():
    """'host' holds the same bits as 'device'; ``batch=2`` runs the receiver solves in pairs, bit-identical for
    multigrid (the guarantee of ``solve_batch``); ``release()`` gives everything back."""
    import torch
    grid, model = small_model('HTI')
    rng = np.random.default_rng(61)
    v = rng.standard_normal((2,) + tuple(grid.shape_cells))
    opts = dict(tol=TOL, sslsolver=False)
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    res = {}
    for name, kw in (('device', {}), ('host', dict(keep='host')), ('batch', dict(batch=2))):
        rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, solver_opts=opts, tol_gradient=TOL, **kw)
        y = _random_data(np.random.default_rng(67), rec.pairs, len(RECS))
        res[name] = (rec.jvec(v), rec.jtvec(y))
        assert rec.n_solves == {'forward': 2, 'receiver': 3, 'jvec': 0, 'jtvec': 0}
        assert rec.kept_bytes == 5 * grid.n_edges * 16
        if name == 'host':
            assert all(t.device.type == 'cpu' and t.is_pinned() for st in rec._stacks.values() for t in st)
        if name == 'batch':
            assert rec._receiver_chunks() == [[0, 1], [2]]
        held = torch.cuda.memory_allocated()
        rec.release()
        gc.collect()
        torch.cuda.synchronize()
        after = torch.cuda.memory_allocated()
        record(f"release(), {name}: allocated {held:,} B -> {after:,} B; before construction {before:,} B")
        assert rec.kept_bytes == 0 and after == before
    for name in ('host', 'batch'):
        same = (all(np.array_equal(res[name][0][p], res['device'][0][p]) for p in res['device'][0]) and
                np.array_equal(res[name][1], res['device'][1]))
        record(f"{name} vs keep='device', batch=1: jvec {_maxdiff(res[name][0], res['device'][0]):.2e}, jtvec "
               f"{_maxdiff(res[name][1], res['device'][1]):.2e}; bit-identical: {same}")
        assert same


@pytest.mark.gpu
def test_linearity_and_the_zero_vector():
    grid, model, lin, rec, v, y, out = _both('HTI')
    zero = rec.jvec(np.zeros_like(v))
    assert all(np.array_equal(zero[p], np.zeros(len(RECS), dtype=complex)) for p in rec.pairs)
    assert np.array_equal(rec.jtvec({}), np.zeros_like(v))
    v1, v2 = np.random.default_rng(41).standard_normal((2,) + v.shape)
    a, b = 0.7, -2.3
    j1, j2, j12 = rec.jvec(v1), rec.jvec(v2), rec.jvec(a * v1 + b * v2)
    combo = {p: a * j1[p] + b * j2[p] for p in j1}
    record(f"linearity: jvec(a v1 + b v2) vs a jvec(v1) + b jvec(v2): {_maxdiff(j12, combo):.2e} (bound 1e-12)")
    assert _maxdiff(j12, combo) <= 1e-12
