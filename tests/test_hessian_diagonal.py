"""Diagonal of the Gauss-Newton Hessian without solves: the kernel ``emg3d_dev_hessian_diagonal`` of
``csrc/hessian.h`` through the C ABI against NumPy written out in this file, and
``gradient.ReciprocalSensitivity.hessian_diagonal`` / ``hessian_vec`` against the existing ``jtvec`` / ``jvec`` of the
same object.

The criterion of every comparison is derived, not tuned. Per cell and row p, with the pairs' sums of magnitudes
``S_{s,r} = sum_{d: row[d] = p} sum_{k in E_d(c)} |e_s[k]| |x_r[k]|`` and ``B = sum_{s,r} w scale (V / 4)^2 S_{s,r}^2``,

    |got - want| <= (ns nr + 48) eps B

holds for ANY order of summation: 16 eps on each twelve-term complex sum, hence 3 * 16 eps S^2 on the square of the
perturbed modulus, and ns nr eps for the outer sum of non-negative terms. The kernel adds to an ``h`` that holds random
values of magnitude <= B / 2 (where B = 0: standard normal values, which must come back bit for bit), so the rounding of
that last addition, eps / 2 * 3 / 2 B on either side, stays inside what the three terms above leave unused (the
twelve-term sums take 14 of their 16 eps).

Inputs, the small survey and the recorder come from ``test_sensitivity``, the device helpers and the NaN-padded stacks
from ``test_reciprocal``.
"""
import functools

import numpy as np
import pytest

from emg3d_amd import _lib, gradient
from test_reciprocal import _comp_grid, _dev, _stack, _up
from test_sensitivity import ADJOINT_CASES, EPS, FREQS, MU_0, OPTS, RECS, SRCS, TOL, _stretched, record, small_model

ROW_MAPS = {'isotropic': (0, 0, 0), 'HTI': (0, 1, 0), 'VTI': (0, 0, 1), 'triaxial': (0, 1, 2)}


# ------------------------------------------------------------------------ the checker ---
def pair_sums(E, X, shape):
    """``Z[d][ix, iy, iz, s, r] = sum over the four d-edges k of the cell of E[s, k] X[r, k]`` for d = x, y, z; the
    fields are laid out [x-edges | y-edges | z-edges], x fastest."""
    nx, ny, nz = shape
    o1 = nx * (ny + 1) * (nz + 1)
    o2 = o1 + (nx + 1) * ny * (nz + 1)
    n = o2 + (nx + 1) * (ny + 1) * nz
    P = np.moveaxis(E[:, None, :n] * X[None, :, :n], -1, 0)               # (n, ns, nr)
    tail = P.shape[1:]
    px = P[:o1].reshape((nx, ny + 1, nz + 1) + tail, order='F')
    py = P[o1:o2].reshape((nx + 1, ny, nz + 1) + tail, order='F')
    pz = P[o2:].reshape((nx + 1, ny + 1, nz) + tail, order='F')
    Z = [0, 0, 0]
    for b in (0, 1):
        for a in (0, 1):
            Z[0] = Z[0] + px[:, a:ny + a, b:nz + b]
            Z[1] = Z[1] + py[a:nx + a, :, b:nz + b]
            Z[2] = Z[2] + pz[a:nx + a, b:ny + b, :]
    return Z


def diagonal_and_bound(Z, S, W, rows, scale, vol3):
    """``scale (V / 4)^2 sum_{s,r} W | sum_{d: rows[d] = p} Z_d |^2`` per row p and cell, (max(rows) + 1, nx, ny, nz),
    and the same with ``S`` (sums of magnitudes) in the place of ``Z``: the B of the module docstring."""
    f = scale * (vol3 / 4) ** 2
    want, B = (np.zeros((max(rows) + 1,) + vol3.shape) for _ in range(2))
    for p in range(max(rows) + 1):
        z, s = (sum(A[d] for d in range(3) if rows[d] == p) for A in (Z, S))
        want[p] = f * np.sum(W * np.abs(z) ** 2, axis=(-2, -1))
        B[p] = f * np.sum(W * s ** 2, axis=(-2, -1))
    return want, B


# ----------------------------------------------------------------------- not gpu tests ---
def test_declared_symbol_and_methods():
    name = 'emg3d_dev_hessian_diagonal'
    assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name) and name + '(' in open(_lib.HEADER).read()
    assert callable(gradient.ReciprocalSensitivity.hessian_diagonal)
    assert callable(gradient.ReciprocalSensitivity.hessian_vec)
    assert not hasattr(gradient.Sensitivity, 'hessian_diagonal')           # no receiver fields: no such method


def test_weights_are_validated_before_any_gpu_work():
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    v = np.ones(grid.shape_cells)
    bad = {'shape': {('a', 'f'): np.ones(len(RECS) + 1)}, 'scalar': {('b', 'f'): 1.0},
           'complex': {('a', 'f'): np.ones(len(RECS), dtype=complex)}, 'negative': {('a', 'f'): np.array([1., -1e-300, 2.])}}
    for what, w in bad.items():
        with pytest.raises(ValueError, match=r"`weights\[\('[ab]', 'f'\)\]` must"):
            rec.hessian_diagonal(w)
        with pytest.raises(ValueError, match=r"`weights\[\('[ab]', 'f'\)\]` must"):
            rec.hessian_vec(v, w)
    with pytest.raises(ValueError, match="`vector` must be real"):
        rec.hessian_vec(np.ones(grid.shape_cells[:2]))
    assert rec.n_solves == {'forward': 0, 'receiver': 0, 'jvec': 0, 'jtvec': 0} and rec.kept_bytes == 0


def test_another_computational_grid_is_refused():
    grid, model = small_model()
    for grids in (_comp_grid(), {('b', 'f'): _comp_grid(), ('a', 'f'): _comp_grid()}):
        rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, grids=grids)
        with pytest.raises(NotImplementedError, match="`grids`"):
            rec.hessian_diagonal()
        assert rec.n_solves['forward'] == 0


def test_no_cpu_fallback_without_gpu():
    if _lib.lib().emg3d_device_count() > 0:
        pytest.skip("GPU present")
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.hessian_diagonal()
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.hessian_vec(np.ones(grid.shape_cells))


# ------------------------------------------------------------------- kernel on the gpu ---
# a workgroup owns 16 x 4 x 4 cells: (67, 5, 9) and (19, 6, 7) exceed that along every axis by a ragged remainder;
# it works on tiles of 4 sources x 4 receivers: (6, 7) is a full and a ragged tile either way
SHAPES = [(1, 1, 1), (5, 3, 2), (67, 5, 9), (12, 10, 8), (19, 6, 7)]
PAIRS = [(1, 1), (3, 5), (9, 2), (4, 4), (6, 7)]


@functools.lru_cache(maxsize=2)
def _kernel_inputs(shape, ns, nr, is_complex):
    """Stacks (host, NaN-padded, and device), volumes, weights with exact zeros, and the checker's Z and S: once for
    the four row maps."""
    grid = _stretched(*shape)
    rng = np.random.default_rng(1000 * sum(shape) + 10 * ns + nr + is_complex)
    (E, es), (X, xs) = _stack(rng, ns, grid.n_edges, is_complex), _stack(rng, nr, grid.n_edges, is_complex)
    W = rng.uniform(0.1, 2.0, (ns, nr))
    W[rng.random((ns, nr)) < 0.3] = 0.0
    vol = grid.cell_volumes.astype(np.float64)
    n = grid.n_edges
    Z, S = pair_sums(E[:, :n], X[:, :n], shape), pair_sums(np.abs(E[:, :n]), np.abs(X[:, :n]), shape)
    return dict(E=_up(E), es=es, X=_up(X), xs=xs, W=W, Wd=_up(W), vol=_up(vol), vol3=vol.reshape(shape, order='F'), Z=Z, S=S)


def _call(inp, shape, ns, nr, is_complex, rows, scale, h, hs):
    from emg3d_amd._device import _ptr, _stream
    _lib.check(_lib.lib().emg3d_dev_hessian_diagonal(
        *shape, int(is_complex), _ptr(inp['E']), inp['es'], ns, _ptr(inp['X']), inp['xs'], nr, _ptr(inp['Wd']), *rows, scale,
        _ptr(inp['vol']), _ptr(h), hs, _stream()), 'emg3d_dev_hessian_diagonal')
    return h.cpu().numpy().reshape(-1, hs)


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(ROW_MAPS))
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('ns, nr', PAIRS)
@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_vs_numpy(shape, ns, nr, is_complex, case):
    """The bound of the module docstring per cell and row; ``h`` starts from random values and has NaN behind each row
    (stride > n_cells), which must survive; a second call on the same inputs gives the same bits."""
    rows = ROW_MAPS[case]
    inp = _kernel_inputs(shape, ns, nr, is_complex)
    ncell, nrows = int(np.prod(shape)), max(rows) + 1
    scale = 0.37
    contribution, B = diagonal_and_bound(inp['Z'], inp['S'], inp['W'], rows, scale, inp['vol3'])
    rng = np.random.default_rng(7 + len(case))
    h0 = np.where(B > 0, rng.uniform(-0.5, 0.5, B.shape) * B, rng.standard_normal(B.shape))
    want = h0 + contribution
    hs = ncell + 5
    start = np.full((nrows, hs), np.nan)
    start[:, :ncell] = np.stack([r.ravel('F') for r in h0])
    got = _call(inp, shape, ns, nr, is_complex, rows, scale, _up(start), hs)
    assert np.all(np.isnan(got[:, ncell:])) and not np.any(np.isnan(got[:, :ncell]))
    got3 = np.stack([r.reshape(shape, order='F') for r in got[:, :ncell]])
    bound = (ns * nr + 48) * EPS * B
    diff = np.abs(got3 - want)
    worst = float(np.max(diff[B > 0] / bound[B > 0])) if np.any(B > 0) else 0.0
    record(f"hessian_diagonal {shape} ns={ns} nr={nr} complex={is_complex} {case}: max |diff| / bound = {worst:.2e} "
           f"(bound (ns nr + 48) eps B); cells with B = 0: {int(np.sum(B == 0))}")
    assert np.all(diff <= bound)
    again = _call(inp, shape, ns, nr, is_complex, rows, scale, _up(start), hs)
    assert np.array_equal(got, again, equal_nan=True)


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    """Every one of them with ``EMG3D_ERR_BADARG`` (-1) before anything is launched."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    a = torch.zeros(64, dtype=torch.complex128, device=_dev())             # a 2 x 2 x 2 grid: 54 edges, 8 cells
    w, vol, d = (torch.zeros(n, dtype=torch.float64, device=_dev()) for n in (1, 8, 24))   # h: three rows of 8 cells
    p, st = _ptr(a), _stream()
    good = dict(nx=2, ny=2, nz=2, c=1, e=p, es=54, ns=1, x=p, xs=54, nr=1, w=_ptr(w), rx=0, ry=1, rz=2, scale=1.0,
                vol=_ptr(vol), h=_ptr(d), hs=8)

    def call(**kw):
        k = {**good, **kw}
        return L.emg3d_dev_hessian_diagonal(k['nx'], k['ny'], k['nz'], k['c'], k['e'], k['es'], k['ns'], k['x'], k['xs'],
                                            k['nr'], k['w'], k['rx'], k['ry'], k['rz'], k['scale'], k['vol'], k['h'], k['hs'],
                                            st)
    bad = [dict(e=None), dict(x=None), dict(w=None), dict(vol=None), dict(h=None), dict(nx=0), dict(ny=0), dict(nz=-1),
           dict(ns=0), dict(nr=0), dict(es=53), dict(xs=53), dict(rx=3), dict(ry=-1), dict(rz=3), dict(hs=7),
           dict(nx=1, ny=4 * 65535 + 1, nz=1, es=10 ** 8, xs=10 ** 8, hs=10 ** 8),       # more than 65 535 workgroups along y
           dict(nx=1, ny=1, nz=4 * 65535 + 1, es=10 ** 8, xs=10 ** 8, hs=10 ** 8)]
    for kw in bad:
        assert call(**kw) == -1, kw
        with pytest.raises(_lib.Emg3dAmdError, match="hessian_diagonal: "):
            _lib.check(call(**kw), 'emg3d_dev_hessian_diagonal')
    torch.cuda.synchronize()
    assert float(d.abs().sum()) == 0.0 and float(a.abs().sum()) == 0.0
    _lib.check(call(), 'emg3d_dev_hessian_diagonal')                        # (the good call is one)


# -------------------------------------------------------------------- method on the gpu ---
METHOD_CASES = {name: ADJOINT_CASES[name] for name in ('isotropic-resistivity', 'HTI', 'VTI', 'triaxial-LgResistivity',
                                                        'magnetic-receiver')}
METHOD_CASES['laplace'] = dict(case='isotropic', mapping='Resistivity', freqs={'f': -1.0})


def _weights(rng):
    """Random weights with one NaN; the pair ('b', 'f') is missing."""
    w = {('a', 'f'): rng.uniform(0.1, 2.0, len(RECS))}
    w[('a', 'f')][1] = np.nan
    return w


@functools.lru_cache(maxsize=None)
def _method(name):
    """One case, once: the object, the weights, ``hessian_diagonal``, the same from 2 ns nr calls of the existing
    ``jtvec``, the bound of the module docstring times chain^2 (per entry of the result), and the solve counts before
    and after."""
    spec = METHOD_CASES[name]
    grid, model = small_model(spec['case'], spec['mapping'])
    freqs = spec.get('freqs', FREQS)
    rec = gradient.ReciprocalSensitivity(model, SRCS, freqs, RECS, solver_opts=OPTS, tol_gradient=TOL,
                                         magnetic=spec.get('magnetic'))
    rec.forward()
    before = dict(rec.n_solves)
    w = _weights(np.random.default_rng(71))
    H = rec.hessian_diagonal(w)
    after = dict(rec.n_solves)
    is_complex = freqs['f'] > 0
    W = np.stack([np.nan_to_num(w.get(p, np.zeros(len(RECS)))) for p in rec.pairs])
    rowwise = np.zeros_like(H)
    for s, pair in enumerate(rec.pairs):
        for r in range(len(RECS)):
            if W[s, r] > 0:
                unit = np.zeros(len(RECS), dtype=complex)
                unit[r] = 1.0
                rowwise += W[s, r] * rec.jtvec({pair: unit}) ** 2
                if is_complex:
                    rowwise += W[s, r] * rec.jtvec({pair: 1j * unit}) ** 2
    E, X = (t.cpu().numpy() for t in rec._stacks['f'])
    shape = tuple(grid.shape_cells)
    smu0 = 2j * np.pi * freqs['f'] * MU_0 if is_complex else -freqs['f'] * MU_0
    S = pair_sums(np.abs(E), np.abs(X), shape)
    _, B = diagonal_and_bound(S, S, W, ROW_MAPS[spec['case']], abs(smu0) ** 2, grid.cell_volumes.reshape(shape, order='F'))
    chain = np.stack([gradient._DCHAIN[spec['mapping']](np.ones(shape), np.asarray(getattr(model, prop), dtype=float))
                      for prop in gradient._PROPS[spec['case']]])
    bound = ((len(SRCS) * len(RECS) + 48) * EPS * B * chain ** 2).reshape(H.shape)
    return dict(grid=grid, model=model, rec=rec, w=w, H=H, rowwise=rowwise, bound=bound, before=before, after=after)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(METHOD_CASES))
def test_method_equals_the_row_by_row_route(name):
    """``hessian_diagonal(w) == sum_i w_i (jtvec(unit_i)^2 + jtvec(1j unit_i)^2)`` (real fields: the first term) within
    twice the bound times chain^2 -- both sides round, both read the same kept fields, so no solver tolerance enters."""
    m = _method(name)
    H, rowwise, bound, rec = m['H'], m['rowwise'], m['bound'], m['rec']
    n = gradient._NCOMP[METHOD_CASES[name]['case']]
    shape = tuple(m['grid'].shape_cells)
    assert H.shape == (shape if n == 1 else (n,) + shape) == rec.jtvec({}).shape and H.flags.f_contiguous
    assert np.all(H >= 0) and np.all(bound > 0)
    worst = float(np.max(np.abs(H - rowwise) / (2 * bound)))
    record(f"hessian_diagonal vs row by row, {name}: max |diff| / (2 bound) = {worst:.2e}; max relative "
           f"{float(np.max(np.abs(H - rowwise) / np.max(H))):.2e}; n_solves {m['before']} -> {m['after']}")
    assert m['before'] == m['after'] == {'forward': 2, 'receiver': 3, 'jvec': 0, 'jtvec': 0}
    assert np.all(np.abs(H - rowwise) <= 2 * bound)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['HTI', 'triaxial-LgResistivity'])
def test_hessian_vec_of_a_unit_vector_gives_the_diagonal(name):
    """Corners, interior, every property row: ``hessian_vec(unit vector of entry c, w)[c] == hessian_diagonal(w)[c]``
    within three times the bound (the unit vector touches twelve edges: twelve non-zero terms in ``dots``)."""
    m = _method(name)
    rec, H, bound = m['rec'], m['H'], m['bound']
    before = dict(rec.n_solves)
    cells = [(0, 0, 0), (9, 9, 7), (9, 0, 7), (0, 9, 0), (4, 5, 3), (6, 2, 5)]
    worst = 0.0
    for k, cell in enumerate(cells):
        c = (k % H.shape[0],) + cell
        v = np.zeros(H.shape)
        v[c] = 1.0
        hv = rec.hessian_vec(v, m['w'])
        assert hv.shape == H.shape
        worst = max(worst, abs(hv[c] - H[c]) / (3 * bound[c]))
        assert abs(hv[c] - H[c]) <= 3 * bound[c], (c, hv[c], H[c], bound[c])
    record(f"hessian_vec(unit)[c] vs hessian_diagonal[c], {name}: max |diff| / (3 bound) = {worst:.2e} over {len(cells)} "
           f"entries")
    assert rec.n_solves == before


@pytest.mark.gpu
def test_host_kept_fields_and_default_weights():
    """``keep='host'`` gives the bits of ``keep='device'``; ``weights=None`` the bits of all-ones weights."""
    m = _method('VTI')
    spec = METHOD_CASES['VTI']
    host = gradient.ReciprocalSensitivity(m['model'], SRCS, FREQS, RECS, solver_opts=OPTS, tol_gradient=TOL, keep='host')
    assert np.array_equal(host.hessian_diagonal(m['w']), m['H'])
    assert host.n_solves == {'forward': 2, 'receiver': 3, 'jvec': 0, 'jtvec': 0}
    host.release()
    rec = m['rec']
    ones = {pair: np.ones(len(RECS)) for pair in rec.pairs}
    H1 = rec.hessian_diagonal()
    assert np.array_equal(H1, rec.hessian_diagonal(ones)) and not np.array_equal(H1, m['H'])
    v = np.random.default_rng(73).standard_normal(H1.shape)
    assert np.array_equal(rec.hessian_vec(v), rec.hessian_vec(v, ones))
    assert np.array_equal(rec.hessian_diagonal({}), np.zeros(H1.shape)) and spec['case'] == 'VTI'
