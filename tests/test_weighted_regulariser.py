"""The weighted / sparse-norm (IRLS) regulariser: ``emg3d_dev_model_regulariser_weighted``,
``emg3d_dev_model_regulariser_weighted_diagonal`` and the ``_rd`` siblings of the block PCG kernels against NumPy in
``longdouble`` written out in this file and, bit for bit, against the plain entry points;
``ReciprocalSensitivity.regulariser_vec_block`` / ``gauss_newton_solve`` with ``cell_weights``, ``norms``,
``linearise_at`` and ``irls_eps`` against dense matrices.

The checker of the plain operator, the layouts and the dense systems come from ``test_gauss_newton_solve``, the small
survey and the recorder from ``test_sensitivity``, the device helpers from ``test_reciprocal``.

The bound of an output of the weighted operator. ``test_gauss_newton_solve`` allows 16 eps of the sum of the magnitudes of
the terms for the plain operator (14 roundings of half an eps each). A weighted coefficient carries in addition

    the sum of the two weights, its product with the coefficient, the product with rho              3 roundings
    rho = (t^2 + eps^2)^(p / 2 - 1): t = (u[c] - u[c']) / l_f carries the difference, l_f and the
    division (3), t^2 twice that, t^2 + eps^2 one more for the square and one for the sum; a
    relative error d of t^2 + eps^2 changes rho by |p / 2 - 1| d <= d                              <= 8 roundings

and the error of the power itself: none for p = 2 (rho is 1, nothing is multiplied), the square root and the division
for p = 1 and the division for p = 0 (correctly rounded: P = 2), and P = 16 for every other p, the loosest a conforming
``pow`` may be (OpenCL full profile: 16 ulp) -- a cap, not a tuning knob. As the issue counts them -- the weight sum, its
product, the difference, the division, the square, the sum with eps^2, the product with rho -- C = 7 eps cover the 11
half-eps above with room to spare; with all norms 2 only the first two occur, C = 2. Per output

    |got - want| <= (16 + C + P) eps (|beta q| + |lam| sum |terms of R p|),

per column ``|<p,q> - want| <= (N + 16) eps sum |p| |q|`` as in ``test_gauss_newton_solve``.
"""
import functools
import itertools

import numpy as np
import pytest

from emg3d_amd import _lib, gradient
from test_gauss_newton_solve import (ALPHAS, KC, LD, REG, TOL, VECTORS, ZERO, _columns, _dense, _diagonal, _flat,
                                     _from_model, _masks, _padded, _pcg, _pcg_numpy, _regulariser, _to_model, _widths,
                                     _z_numpy, regulariser_numpy)
from test_reciprocal import _dev, _up
from test_sensitivity import EPS, FREQS, RECS, SRCS, record, small_model

SYMBOLS = ('emg3d_dev_model_regulariser_weighted', 'emg3d_dev_model_regulariser_weighted_diagonal',
           'emg3d_dev_pcg_update_rd', 'emg3d_dev_pcg_direction_rd')
BADARG = -1
NORMS = [(2.0, 2.0, 2.0, 2.0), (1.0, 1.0, 1.0, 1.0), (0.0, 2.0, 1.0, 0.5)]
THRESHOLDS = [(1e-3, 1e-3), (0.5, 0.25)]
ALPHA = ALPHAS[-1]


def slack(norms):
    """16 + C + P of the module's docstring."""
    if all(p == 2 for p in norms):
        return 16 + 2
    return 16 + 7 + (2 if all(p in (0, 1, 2) for p in norms) else 16)


# ----------------------------------------------------------------------- not gpu tests ---
def test_symbols_are_declared():
    header = open(_lib.HEADER).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name) and name + '(' in header


def test_methods_take_the_keywords():
    import inspect
    for name in ('regulariser_vec_block', 'gauss_newton_solve'):
        par = inspect.signature(getattr(gradient.ReciprocalSensitivity, name)).parameters
        for key in ('cell_weights', 'norms', 'linearise_at', 'irls_eps'):
            assert par[key].default is None and par[key].kind is inspect.Parameter.KEYWORD_ONLY


def _bad_keywords(shape, n):
    one, u = np.ones(shape), np.zeros(((n,) if n > 1 else ()) + shape)
    sparse = dict(norms=(1, 1, 1, 1), linearise_at=u, irls_eps=(1e-3, 1e-3))
    minus, nan = one.copy(), one.copy()
    minus[0, 0, 0], nan[-1, -1, -1] = -1e-300, np.nan
    return [
        (dict(cell_weights=minus), "`cell_weights` must be real, finite and >= 0"),
        (dict(cell_weights=nan), "`cell_weights` must be real, finite and >= 0"),
        (dict(cell_weights=one.astype(complex)), "`cell_weights` must be real, finite and >= 0"),
        (dict(cell_weights=np.ones(shape[:2])), "`cell_weights` must be real, finite and >= 0"),
        (dict(cell_weights=np.ones((n + 1,) + shape)), "`cell_weights` must be real, finite and >= 0"),
        (dict(norms=(2, 2, 2)), "`norms` must be four"), (dict(norms=(2, 2, 2, 2.5)), "`norms` must be four"),
        (dict(norms=(-0.1, 2, 2, 2)), "`norms` must be four"), (dict(norms=(2, np.nan, 2, 2)), "`norms` must be four"),
        (dict(norms=2.0), "`norms` must be four"),
        (dict(linearise_at=u), "with all four norms 2"), (dict(irls_eps=(1e-3, 1e-3)), "with all four norms 2"),
        (dict(norms=(2, 2, 2, 2), linearise_at=u), "with all four norms 2"),
        (dict(norms=(2, 2, 2, 2), irls_eps=(1e-3, 1e-3)), "with all four norms 2"),
        (dict(norms=(1, 2, 2, 2), irls_eps=(1e-3, 1e-3)), "a norm other than 2 needs"),
        (dict(norms=(2, 2, 0, 2), linearise_at=u), "a norm other than 2 needs"),
        (dict(sparse, linearise_at=np.zeros(shape[:2])), "`linearise_at` must be one real, finite model-shaped"),
        (dict(sparse, linearise_at=np.stack([u, u])), "`linearise_at` must be one real, finite model-shaped"),
        (dict(sparse, linearise_at=u + 1j), "`linearise_at` must be one real, finite model-shaped"),
        (dict(sparse, linearise_at=u + np.inf), "`linearise_at` must be one real, finite model-shaped"),
        (dict(sparse, irls_eps=(1e-3, 0.0)), "`irls_eps` must be two"), (dict(sparse, irls_eps=(-1.0, 1e-3)), "`irls_eps` must be two"),
        (dict(sparse, irls_eps=1e-3), "`irls_eps` must be two"), (dict(sparse, irls_eps=(1e-3, np.inf)), "`irls_eps` must be two"),
    ]


@pytest.mark.parametrize('case', ['isotropic', 'triaxial'])
def test_keywords_are_validated_before_any_gpu_work(case):
    """Every rule of the validation, with "Provided:", without a device; ``n_solves`` and ``kept_bytes`` stay."""
    grid, model = small_model(case)
    shape, n = tuple(grid.shape_cells), gradient._NCOMP[case]
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    vec = np.ones((n,) + shape)
    for kwargs, match in _bad_keywords(shape, n):
        with pytest.raises(ValueError, match=match) as err:
            rec.gauss_newton_solve(vec, [1.0, 10.0], **kwargs)
        assert "Provided:" in str(err.value), kwargs
        with pytest.raises(ValueError, match=match) as err:
            rec.regulariser_vec_block(vec[None], **kwargs)
        assert "Provided:" in str(err.value), kwargs
    assert rec.n_solves == ZERO and rec.kept_bytes == 0


def test_device_tensors_are_validated_before_any_gpu_work():
    import torch
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    vec, ncell = np.ones(grid.shape_cells), grid.n_cells
    for kwargs, match in ((dict(cell_weights=torch.ones(ncell, dtype=torch.float64)), "`cell_weights` on the device"),
                          (dict(cell_weights=torch.ones(ncell + 1, dtype=torch.float64, device='meta')), "`cell_weights` on"),
                          (dict(norms=(1, 1, 1, 1), irls_eps=(1e-3, 1e-3), linearise_at=torch.zeros((1, ncell))),
                           "`linearise_at` on the device")):
        with pytest.raises(ValueError, match=match) as err:
            rec.gauss_newton_solve(vec, [1.0], **kwargs)
        assert "Provided:" in str(err.value)
    assert rec.n_solves == ZERO and rec.kept_bytes == 0


def test_no_cpu_fallback_without_gpu():
    if _lib.lib().emg3d_device_count() > 0:
        pytest.skip("GPU present")
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    one = np.ones(grid.shape_cells)
    kw = dict(cell_weights=one, norms=(1, 1, 1, 1), linearise_at=one, irls_eps=(1e-3, 1e-3))
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.regulariser_vec_block(one[None], **kw)
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.gauss_newton_solve(one, [1.0, 2.0], **kw)
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.gauss_newton_solve(one, [1.0], precondition=False, cell_weights=one)


# ------------------------------------------------------------------------ the checker ---
def rho_numpy(p, eps, t):
    """(t^2 + eps^2)^(p / 2 - 1) in longdouble; exactly 1 for p = 2."""
    if p == 2:
        return np.ones_like(t, dtype=LD)
    return (np.asarray(t, dtype=LD) ** 2 + LD(eps) ** 2) ** (LD(p) / 2 - 1)


def weighted_component_numpy(h, alphas, mask, w, u, norms, eps, v):
    """``R v`` of ONE component in ``longdouble`` for v (nvec, nx, ny, nz) and the sum of the magnitudes of its terms, as
    ``regulariser_numpy``; w: weights (nx, ny, nz) or None, u: linearisation values (nx, ny, nz) or None (all norms 2)."""
    hx, hy, hz = (np.asarray(x, dtype=LD) for x in h)
    nx, ny, nz = len(hx), len(hy), len(hz)
    a = np.ones((nx, ny, nz), dtype=LD) if mask is None else mask.astype(LD)
    w = np.ones((nx, ny, nz), dtype=LD) if w is None else np.asarray(w, dtype=LD)
    u = None if u is None else np.asarray(u, dtype=LD)
    v = np.asarray(v, dtype=LD)
    vol = hx[:, None, None] * hy[None, :, None] * hz[None, None, :]
    cs = LD(alphas[0]) * vol * w * (1 if norms[0] == 2 else rho_numpy(norms[0], eps[0], u))
    out, mag = cs * v, cs * np.abs(v)
    area = (hy[None, :, None] * hz[None, None, :], hx[:, None, None] * hz[None, None, :], hx[:, None, None] * hy[None, :, None])
    for d, x in enumerate((hx, hy, hz)):
        if len(x) < 2:
            continue
        lo = tuple(slice(0, -1) if k == d else slice(None) for k in range(3))
        hi = tuple(slice(1, None) if k == d else slice(None) for k in range(3))
        dist = (0.5 * (x[:-1] + x[1:])).reshape([-1 if k == d else 1 for k in range(3)])
        coef = LD(alphas[1 + d]) * area[d] / dist * a[lo] * a[hi] * (0.5 * (w[lo] + w[hi]))
        if norms[1 + d] != 2:
            coef = coef * rho_numpy(norms[1 + d], eps[1], (u[lo] - u[hi]) / dist)
        vlo, vhi = v[(slice(None),) + lo], v[(slice(None),) + hi]
        out[(slice(None),) + lo] += coef * (vlo - vhi)
        out[(slice(None),) + hi] += coef * (vhi - vlo)
        mag[(slice(None),) + lo] += coef * (np.abs(vlo) + np.abs(vhi))
        mag[(slice(None),) + hi] += coef * (np.abs(vlo) + np.abs(vhi))
    return out * a, mag * a


def weighted_numpy(h, alphas, mask, w, u, norms, eps, v, vpc):
    """The same for v (nvec, nx, ny, nz) whose vector j is component j % vpc: w None, (nx, ny, nz) for all components or
    (vpc, nx, ny, nz); u None or (vpc, nx, ny, nz)."""
    v = np.asarray(v)
    out, mag = np.zeros(v.shape, dtype=LD), np.zeros(v.shape, dtype=LD)
    for k in range(vpc):
        wk = w if w is None or np.ndim(w) == 3 else w[k]
        out[k::vpc], mag[k::vpc] = weighted_component_numpy(h, alphas, mask, wk, None if u is None else u[k], norms, eps,
                                                            v[k::vpc])
    return out, mag


def test_checker_reduces_to_the_plain_one():
    """Weights of 1 and norms of 2: the plain checker, bit for bit; a face's coefficient is the mean of the weights times
    rho of the gradient (one face, by hand)."""
    rng = np.random.default_rng(2)
    shape = (4, 3, 2)
    h = [_widths(n, 30.0, rng) for n in shape]
    v = rng.standard_normal((6,) + shape)
    mask = rng.uniform(size=shape) < 0.8
    a, b = regulariser_numpy(h, ALPHA, mask, v), weighted_numpy(h, ALPHA, mask, np.ones((3,) + shape), None, NORMS[0], None, v, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    h2 = [np.array([2.0, 4.0]), np.array([5.0]), np.array([7.0])]
    w, u = np.array([1.0, 3.0]).reshape(2, 1, 1), np.array([0.5, 2.0]).reshape(1, 2, 1, 1)
    e = np.array([1.0, 0.0]).reshape(1, 2, 1, 1)
    got, _ = weighted_numpy(h2, (0.0, 1.5, 0.0, 0.0), None, w, u, (2, 1, 2, 2), (0.1, 0.2), e, 1)
    want = 1.5 * 35.0 / 3.0 * 2.0 * ((1.5 / 3.0) ** 2 + 0.2 ** 2) ** -0.5
    assert np.allclose(np.asarray(got, dtype=float).ravel(), [want, -want], rtol=1e-14, atol=0)


# ------------------------------------------------------------------ kernels on the gpu ---
def _rows(a, ncell):
    """(rows, nx, ny, nz) -> (device rows of stride n_cells + 3 with NaN between and behind them, the stride)."""
    stride = ncell + 3
    out = np.full((len(a), stride), np.nan)
    out[:, :ncell] = _flat(a)
    return _up(out), stride


def _weights_up(w, ncell):
    """w None, (nx, ny, nz) or (vpc, nx, ny, nz) -> (tensor or None, stride), every row followed by NaN."""
    if w is None:
        return None, 0
    if np.ndim(w) == 3:
        return _padded(w.ravel(order='F')), 0
    return _rows(w, ncell)


def _weighted_raw(h, alphas, mask, w, u, norms, eps, nvec, vpc, pd, qd, beta, ld, pq, ws, ws_len, strides=None):
    """The status of ``emg3d_dev_model_regulariser_weighted`` on device buffers."""
    from emg3d_amd._device import _ptr, _stream
    nx, ny, nz = (len(x) for x in h)
    ncell = nx * ny * nz
    hd = [_padded(x) for x in h]
    md = None if mask is None else _up(np.concatenate([mask.ravel(order='F').astype(np.uint8), np.full(7, 1, np.uint8)]))
    wd, wstride = _weights_up(w, ncell)
    ud, ustride = (None, 0) if u is None else _rows(u, ncell)
    if strides is not None:
        wstride, ustride = strides
    eps = (0.0, 0.0) if eps is None else eps
    return _lib.lib().emg3d_dev_model_regulariser_weighted(
        nx, ny, nz, _ptr(hd[0]), _ptr(hd[1]), _ptr(hd[2]), *[float(x) for x in alphas], None if md is None else _ptr(md),
        None if wd is None else _ptr(wd), wstride, None if ud is None else _ptr(ud), ustride, *[float(x) for x in norms],
        *[float(x) for x in eps], nvec, vpc, _ptr(pd), _ptr(qd), float(beta), None if ld is None else _ptr(ld),
        None if pq is None else _ptr(pq), None if ws is None else _ptr(ws), ws_len, _stream())


def _weighted(h, alphas, mask, w, u, norms, eps, p, q0, beta, lam, vpc, with_pq=True):
    """The weighted kernel on p (nvec, nx, ny, nz), as ``_regulariser`` of ``test_gauss_newton_solve``: (q (nvec, n_cells),
    pq (ncol,) or None); every buffer NaN behind its end."""
    import torch
    L = _lib.lib()
    nx, ny, nz = (len(x) for x in h)
    nvec, ncell, ncol = len(p), nx * ny * nz, len(p) // vpc
    pd = _padded(_flat(p))
    qd = _padded(np.full((nvec, ncell), np.nan) if q0 is None else q0)
    ld = None if lam is None else _padded(lam)
    ws_len = L.emg3d_model_regulariser_ws_len(nx, ny, nz, nvec, vpc)
    assert ws_len > 0
    ws = torch.full((ws_len,), float('nan'), dtype=torch.float64, device=_dev())
    pq = torch.full((ncol + 2,), float('nan'), dtype=torch.float64, device=_dev())
    _lib.check(_weighted_raw(h, alphas, mask, w, None if u is None else u[:vpc], norms, eps, nvec, vpc, pd, qd, beta, ld,
                             pq if with_pq else None, ws if with_pq else None, ws_len if with_pq else 0),
               'emg3d_dev_model_regulariser_weighted')
    q = qd.cpu().numpy()
    assert np.all(np.isnan(q[nvec * ncell:])) and np.all(np.isnan(pq.cpu().numpy()[ncol:]))     # nothing behind the end
    return q[:nvec * ncell].reshape(nvec, ncell), (pq.cpu().numpy()[:ncol] if with_pq else None)


def _weighted_diagonal(h, alphas, mask, w, u, norms, eps, vpc):
    import torch
    from emg3d_amd._device import _ptr, _stream
    nx, ny, nz = (len(x) for x in h)
    ncell = nx * ny * nz
    hd = [_padded(x) for x in h]
    md = None if mask is None else _up(mask.ravel(order='F').astype(np.uint8))
    wd, wstride = _weights_up(w, ncell)
    ud, ustride = (None, 0) if u is None else _rows(u[:vpc], ncell)
    eps = (0.0, 0.0) if eps is None else eps
    out = torch.full((vpc * ncell + 3,), float('nan'), dtype=torch.float64, device=_dev())
    _lib.check(_lib.lib().emg3d_dev_model_regulariser_weighted_diagonal(
        nx, ny, nz, _ptr(hd[0]), _ptr(hd[1]), _ptr(hd[2]), *[float(x) for x in alphas], None if md is None else _ptr(md),
        None if wd is None else _ptr(wd), wstride, None if ud is None else _ptr(ud), ustride, *[float(x) for x in norms],
        *[float(x) for x in eps], vpc, _ptr(out), _stream()), 'emg3d_dev_model_regulariser_weighted_diagonal')
    out = out.cpu().numpy()
    assert np.all(np.isnan(out[vpc * ncell:])) and not np.any(np.isnan(out[:vpc * ncell]))
    return out[:vpc * ncell].reshape(vpc, ncell)


def _fields(rng, shape):
    """Weights (3, nx, ny, nz) >= 0 with exact zeros and linearisation values (3, nx, ny, nz), standard normal, some
    neighbours along every direction exactly equal (t = 0)."""
    w = rng.uniform(0.2, 5.0, (3,) + shape) * (rng.uniform(size=(3,) + shape) > 0.15)
    u = rng.standard_normal((3,) + shape)
    for d in range(3):
        if shape[d] > 1:
            lo = tuple(slice(0, -1) if k == d + 1 else slice(None) for k in range(4))
            hi = tuple(slice(1, None) if k == d + 1 else slice(None) for k in range(4))
            same = rng.uniform(size=u[lo].shape) < 0.1
            u[hi] = np.where(same, u[lo], u[hi])
    return w, u


SHAPES = dict(argnames='nx, ny, nz', argvalues=[(nx, ny, nz) for nx in (1, 2, 63, 64, 65, 130)
                                                 for ny, nz in ((1, 1), (2, 5), (5, 2))])


@pytest.mark.gpu
@pytest.mark.parametrize(**SHAPES)
def test_weighted_regulariser_vs_numpy(nx, ny, nz):
    """Per output and per column the bounds of the module's docstring. All combinations of the vector layouts, the masks,
    weights shared by the components and per component (with exact zeros), the norms, the thresholds (which only norms
    other than 2 read), beta and lambda; u is standard normal with equal neighbours; every buffer, the weights and u
    included, is followed by NaN. Rows of inactive cells are exactly 0."""
    rng = np.random.default_rng(2000 * nx + 10 * ny + nz)
    h = [_widths(nx, 40.0, rng), _widths(ny, 55.0, rng), _widths(nz, 25.0, rng)]
    shape, ncell = (nx, ny, nz), nx * ny * nz
    w3, u3 = _fields(rng, shape)
    worst = {norms: [0.0, 0.0] for norms in NORMS}
    settings = [(NORMS[0], None)] + [(norms, eps) for norms in NORMS[1:] for eps in THRESHOLDS]
    for (nvec, vpc), mask, shared, (norms, eps), beta, use_lam in itertools.product(
            VECTORS, _masks(rng, shape), (True, False), settings, (0.0, 1.0), (False, True)):
        ncol = nvec // vpc
        w = w3[0] if shared else w3[:vpc]
        u = None if eps is None else u3
        p = rng.standard_normal((nvec,) + shape)
        q0 = rng.standard_normal((nvec, ncell)) if beta else None
        lam = 10 ** rng.uniform(-2, 2, ncol) if use_lam else None
        got, pq = _weighted(h, ALPHA, mask, w, u, norms, eps, p, q0, beta, lam, vpc)
        rp, mag = weighted_numpy(h, ALPHA, mask, w, u, norms, eps, p, vpc)
        lcol = np.repeat(np.ones(ncol) if lam is None else lam, vpc).astype(LD)[:, None]
        want = lcol * _flat(rp) + (beta * q0.astype(LD) if beta else 0)
        bound = slack(norms) * EPS * (lcol * _flat(mag) + (np.abs(beta * q0) if beta else 0))
        tag = (nvec, vpc, mask is not None, shared, norms, eps, beta, use_lam)
        assert not np.any(np.isnan(got)), tag
        err = np.abs(got - want)
        some = bound > 0
        ratio = float(np.max(err[some] / bound[some], initial=0.0))
        print(f"weighted regulariser {shape} {tag}: max |diff| / bound = {ratio:.2e}")
        assert np.all(err <= bound), tag
        if mask is not None and not beta:
            assert np.all(got[:, ~mask.ravel(order='F')] == 0.0)          # rows of inactive cells: exactly 0
        pf = _flat(p).astype(LD)
        want_pq = np.sum((pf * got.astype(LD)).reshape(ncol, -1), axis=1)
        bound_pq = (vpc * ncell + 16) * EPS * np.sum(np.abs(pf * got).reshape(ncol, -1), axis=1)
        assert np.all(np.abs(pq - want_pq) <= bound_pq), tag
        some = bound_pq > 0
        worst[norms][0] = max(worst[norms][0], ratio)
        worst[norms][1] = max(worst[norms][1], float(np.max(np.abs(pq - want_pq)[some] / bound_pq[some], initial=0.0)))
    for norms in NORMS:
        record(f"weighted regulariser {nx} x {ny} x {nz} norms {norms}: max |diff| / bound = {worst[norms][0]:.2e} "
               f"({slack(norms)} eps sum |terms|), <p,q> {worst[norms][1]:.2e} ((N + 16) eps)")


@pytest.mark.gpu
@pytest.mark.parametrize(**SHAPES)
def test_bits_of_the_plain_operator(nx, ny, nz):
    """No weights, or weights that are all exactly 1.0 (one array, or one per component), and all norms 2: q, <p,q> and
    the diagonal have the bits of ``emg3d_dev_model_regulariser`` / ``_diagonal``. The same weighted call twice, with and
    without <p,q>: the same bits."""
    rng = np.random.default_rng(3000 * nx + 10 * ny + nz)
    h = [_widths(nx, 40.0, rng), _widths(ny, 55.0, rng), _widths(nz, 25.0, rng)]
    shape, ncell = (nx, ny, nz), nx * ny * nz
    for (nvec, vpc), mask, (beta, use_lam) in itertools.product(VECTORS, _masks(rng, shape), ((0.0, False), (1.0, True))):
        p = rng.standard_normal((nvec,) + shape)
        q0 = rng.standard_normal((nvec, ncell)) if beta else None
        lam = 10 ** rng.uniform(-2, 2, nvec // vpc) if use_lam else None
        want = _regulariser(h, ALPHA, mask, p, q0, beta, lam, vpc)
        for w in (None, np.ones(shape), np.ones((vpc,) + shape)):
            got = _weighted(h, ALPHA, mask, w, None, NORMS[0], None, p, q0, beta, lam, vpc)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (nvec, vpc, beta, np.ndim(w))
    for mask in _masks(rng, shape):
        want = _diagonal(h, ALPHA, mask)
        for vpc, w in ((1, None), (3, None), (2, np.ones(shape)), (3, np.ones((3,) + shape))):
            got = _weighted_diagonal(h, ALPHA, mask, w, None, NORMS[0], None, vpc)
            assert all(np.array_equal(row, want) for row in got)
    w3, u3 = _fields(rng, shape)                           # (the last layout of the loop: nine vectors, three per column)
    some = _masks(rng, shape)[1]
    again = [_weighted(h, ALPHA, some, w3, u3, NORMS[2], THRESHOLDS[1], p, q0, beta, lam, vpc, with_pq=x)
             for x in (False, True, True)]
    assert np.array_equal(again[0][0], again[1][0]) and np.array_equal(again[1][0], again[2][0])
    assert np.array_equal(again[1][1], again[2][1])


PROP = dict(shape=(7, 5, 3), norms=(0.5, 1.0, 1.5, 0.0), eps=(0.3, 0.05))


@functools.lru_cache(maxsize=None)
def _property_case():
    rng = np.random.default_rng(17)
    shape = PROP['shape']
    h = [_widths(n, 30.0, rng) for n in shape]
    mask = rng.uniform(size=shape) < 0.8
    w3, u3 = _fields(rng, shape)
    return rng, h, mask, w3, u3


@pytest.mark.gpu
def test_properties():
    """7 x 5 x 3 cells, a mask, weights and the norms (0.5, 1, 1.5, 0). The dense matrix from a block of unit vectors is
    EXACTLY symmetric (every factor of a face is the same from either side); constants are annihilated exactly when
    alpha_s = 0; ``<v, R v> >= 0`` as the kernel sums it; with three components and three different u the diagonal blocks
    differ and each is its own ``longdouble`` operator within the bound of the module's docstring."""
    rng, h, mask, w3, u3 = _property_case()
    shape, norms, eps = PROP['shape'], PROP['norms'], PROP['eps']
    ncell = int(np.prod(shape))
    eye = np.eye(ncell).reshape((ncell,) + shape, order='F')
    for m, w in itertools.product((None, mask), (w3[1], w3)):
        dense, _ = _weighted(h, ALPHA, m, w if np.ndim(w) == 3 else w[:1], u3, norms, eps, eye, None, 0.0, None, 1, False)
        assert np.array_equal(dense, dense.T) and np.count_nonzero(dense) > ncell
        const = np.full((3,) + shape, -3.7)
        got, _ = _weighted(h, (0.0, 1.0, 2.0, 3.0), m, w, u3, norms, eps, const, None, 0.0, None, 3)
        assert np.all(got == 0.0)                                                 # exactly annihilated
        v = rng.standard_normal((6,) + shape)
        _, vrv = _weighted(h, ALPHA, m, w, u3, norms, eps, v, None, 0.0, None, 3)
        assert np.all(vrv >= 0)
        _, vrv = _weighted(h, (0.0, 1.0, 2.0, 3.0), m, w, u3, norms, eps, v, None, 0.0, None, 1)
        assert np.all(vrv >= 0)
    # three components, every column holds the same unit vector in each: got[col * 3 + k] is column col of R_k
    block, _ = _weighted(h, ALPHA, mask, w3, u3, norms, eps, np.repeat(eye, 3, axis=0), None, 0.0, None, 3, False)
    block = block.reshape(ncell, 3, ncell)
    for k in range(3):
        want, mag = weighted_component_numpy(h, ALPHA, mask, w3[k], u3[k], norms, eps, eye)
        assert np.all(np.abs(block[:, k] - _flat(want)) <= slack(norms) * EPS * _flat(mag))
        assert np.array_equal(block[:, k], block[:, k].T)
        assert not np.array_equal(block[:, k], block[:, (k + 1) % 3])
    # rows AND columns of inactive cells: what they hold -- in p, in the weights, in u -- changes nothing
    v = rng.standard_normal((3,) + shape)
    dirty_v, dirty_w, dirty_u = v.copy(), w3.copy(), u3.copy()
    dirty_v[:, ~mask] = dirty_w[:, ~mask] = dirty_u[:, ~mask] = np.nan
    a, _ = _weighted(h, ALPHA, mask, dirty_w, dirty_u, norms, eps, dirty_v, None, 0.0, None, 3, False)
    b, _ = _weighted(h, ALPHA, mask, w3, u3, norms, eps, v, None, 0.0, None, 3, False)
    assert np.array_equal(a, b) and np.all(a[:, ~mask.ravel(order='F')] == 0.0)


@pytest.mark.gpu
def test_diagonal_vs_unit_vectors():
    """The diagonal kernel against the diagonal of the dense ``longdouble`` operator, within the bound of the module's
    docstring, and against the kernel's own dense matrix within twice that; weights shared and per component, one and
    three components; 0 on inactive cells."""
    rng, h, mask, w3, u3 = _property_case()
    shape, eps = PROP['shape'], PROP['eps']
    ncell = int(np.prod(shape))
    eye = np.eye(ncell).reshape((ncell,) + shape, order='F')
    for m, (vpc, w), norms in itertools.product((None, mask), ((1, w3[0]), (3, w3[2]), (3, w3)), (PROP['norms'], NORMS[0], NORMS[2])):
        u = None if norms == NORMS[0] else u3
        got = _weighted_diagonal(h, ALPHA, m, w, u, norms, eps if u is not None else None, vpc)
        for k in range(vpc):
            wk = w if np.ndim(w) == 3 else w[k]
            uk = None if u is None else u[k]
            want, mag = weighted_component_numpy(h, ALPHA, m, wk, uk, norms, eps, eye)
            want, mag = np.diagonal(_flat(want)), np.diagonal(_flat(mag))
            assert np.all(np.abs(got[k] - want) <= slack(norms) * EPS * mag), (vpc, k, norms)
            dense, _ = _weighted(h, ALPHA, m, wk, None if uk is None else uk[None], norms, eps if u is not None else None,
                                 eye, None, 0.0, None, 1, False)
            assert np.all(np.abs(got[k] - np.diagonal(dense)) <= 2 * slack(norms) * EPS * mag)
            if m is not None:
                assert np.all(got[k][~m.ravel(order='F')] == 0.0)


def _pcg_rd(ncell, vpc, K, first, x, r, p, q, hd, rd, stride, mask, table, pq, tol):
    """``_pcg`` of ``test_gauss_newton_solve`` through the ``_rd`` entries; rd: (rows, ncell), rows of the given stride."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    xd, rdv, pd, qd, hdd = (_padded(a) for a in (x, r, p, q, hd))
    rows = np.full((len(rd), max(stride, ncell)), np.nan)
    rows[:, :ncell] = rd
    rdd = _padded(rows) if stride else _padded(rd[0])
    md = None if mask is None else _up(mask.astype(np.uint8))
    td, pqd = _up(table), _padded(pq)
    ws_len = L.emg3d_pcg_ws_len(ncell, K)
    ws = torch.full((ws_len,), float('nan'), dtype=torch.float64, device=_dev())
    opt = (_ptr(hdd), _ptr(rdd), stride, None if md is None else _ptr(md))
    _lib.check(L.emg3d_dev_pcg_update_rd(ncell, vpc, K, first, _ptr(xd), _ptr(rdv), _ptr(pd), _ptr(qd), *opt, _ptr(td),
                                         _ptr(pqd), _ptr(ws), ws_len, _stream()), 'emg3d_dev_pcg_update_rd')
    _lib.check(L.emg3d_dev_pcg_scalar(ncell, K, first, tol, _ptr(td), _ptr(pqd), _ptr(ws), ws_len, _stream()),
               'emg3d_dev_pcg_scalar')
    _lib.check(L.emg3d_dev_pcg_direction_rd(ncell, vpc, K, first, _ptr(pd), _ptr(rdv), *opt, _ptr(td), _stream()),
               'emg3d_dev_pcg_direction_rd')
    n = K * vpc * ncell
    return xd.cpu().numpy()[:n], rdv.cpu().numpy()[:n], pd.cpu().numpy()[:n], td.cpu().numpy()


@pytest.mark.gpu
def test_pcg_kernels_with_a_diagonal_per_component():
    """1025 cells: the grid-stride loop of a workgroup of 256 takes a second step. Stride 0: the bits of
    ``emg3d_dev_pcg_update`` / ``_direction`` on the same inputs. Stride n_cells (and a larger one, NaN between the rows)
    with three different diagonals against NumPy with the bounds of ``test_gauss_newton_solve``: elements 4 eps of the
    magnitudes, sums ``(N + 16) eps sum |r| |z|``."""
    rng = np.random.default_rng(41)
    ncell, vpc, K, tol = 1025, 3, 2, 1e-3
    N = vpc * ncell
    x, r, p, q = rng.standard_normal((4, K, vpc, ncell))
    hd, rd = rng.uniform(0.5, 2.0, (vpc, ncell)), rng.uniform(0.1, 1.0, (vpc, ncell))
    act = rng.uniform(size=ncell) < 0.8
    table = np.zeros((K, 8))
    table[:, 0], table[:, 1], table[:, 2], table[:, 6] = [0.3, 7.0], 1.0, rng.uniform(0.5, 2.0, K), 4
    pq = rng.uniform(0.5, 2.0, K) * 50
    for first in (0, 1):
        want = _pcg(ncell, vpc, K, first, x, r, p, q, hd, rd[0], act, table, pq, tol)
        got = _pcg_rd(ncell, vpc, K, first, x, r, p, q, hd, rd[:1], 0, act, table, pq, tol)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    for stride in (ncell, ncell + 5):
        got = _pcg_rd(ncell, vpc, K, 0, x, r, p, q, hd, rd, stride, act, table, pq, tol)
        gx, gr, gp = (a.reshape(K, vpc, ncell) for a in got[:3])
        gt = got[3]
        assert not any(np.any(np.isnan(a)) for a in got)
        for k in range(K):
            lam, alpha = table[k, 0], table[k, 2] / pq[k]
            assert np.all(np.abs(gx[k] - (x[k] + LD(alpha) * p[k])) <= 4 * EPS * (np.abs(x[k]) + np.abs(alpha * p[k])))
            want_r = np.where(act, r[k] - LD(alpha) * q[k], 0)
            assert np.all(np.abs(gr[k] - want_r) <= 4 * EPS * (np.abs(r[k]) + np.abs(alpha * q[k])))
            z = np.where(act, gr[k].astype(LD) / (hd.astype(LD) + LD(lam) * rd.astype(LD)), 0)      # per component
            shared = _z_numpy(gr[k], act, hd, rd[0], lam)
            assert not np.allclose(np.asarray(z[1:], dtype=float), np.asarray(shared[1:], dtype=float), rtol=1e-3)
            rz, rr = np.sum(gr[k] * z), np.sum(gr[k].astype(LD) ** 2)
            assert abs(gt[k, 2] - rz) <= (N + 16) * EPS * np.sum(np.abs(gr[k] * z))
            assert abs(gt[k, 5] - rr) <= (N + 16) * EPS * rr
            assert gt[k, 7] == 0 and gt[k, 6] == 5
            beta = gt[k, 2] / gt[k, 3]
            assert np.all(np.abs(gp[k] - (z + LD(beta) * p[k])) <= 4 * EPS * (np.abs(z) + np.abs(beta * p[k])))
        again = _pcg_rd(ncell, vpc, K, 0, x, r, p, q, hd, rd, stride, act, table, pq, tol)
        assert all(np.array_equal(a, b) for a, b in zip(got, again))


@pytest.mark.gpu
def test_bad_arguments_write_nothing():
    """Every case that the header lists returns EMG3D_ERR_BADARG with a message; q, pq and the diagonal, filled with NaN,
    stay NaN."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    rng = np.random.default_rng(5)
    shape = (5, 3, 2)
    ncell = int(np.prod(shape))
    h = [_widths(n, 30.0, rng) for n in shape]
    w3, u3 = _fields(rng, shape)
    u4 = np.concatenate([u3, u3[:1]])
    nan = float('nan')
    good = dict(w=w3, u=u3, norms=(1.0, 1.0, 1.0, 1.0), eps=(1e-3, 1e-3), nvec=6, vpc=3, strides=None, h=h, same=False)
    cases = [dict(nvec=8, vpc=4, u=u4, w=None), dict(nvec=7), dict(nvec=0), dict(vpc=0), dict(norms=(2.0, 2.0, 2.5, 2.0)),
             dict(norms=(-0.5, 2.0, 2.0, 2.0)), dict(norms=(2.0, nan, 2.0, 2.0)), dict(norms=(2.0, 2.0, 2.0, float('inf'))),
             dict(u=None), dict(eps=(0.0, 1e-3)), dict(eps=(1e-3, -1.0)), dict(eps=(nan, 1e-3)), dict(eps=(1e-3, float('inf'))),
             dict(strides=(ncell - 1, ncell + 3)), dict(strides=(ncell + 3, 1)), dict(same=True), dict(h=None)]
    for change in cases:
        c = dict(good, **change)
        nvec = max(c['nvec'], 8)
        pd = _up(rng.standard_normal(nvec * ncell))
        qd = torch.full((nvec * ncell,), nan, dtype=torch.float64, device=_dev())
        pq = torch.full((8,), nan, dtype=torch.float64, device=_dev())
        ws = torch.full((4096,), nan, dtype=torch.float64, device=_dev())
        if c['h'] is None:
            hd = _padded(h[0])
            status = L.emg3d_dev_model_regulariser_weighted(
                *shape, _ptr(hd), None, _ptr(hd), *ALPHA, None, None, 0, None, 0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 6, 3,
                _ptr(pd), _ptr(qd), 0.0, None, _ptr(pq), _ptr(ws), 4096, _stream())
        else:
            status = _weighted_raw(h, ALPHA, None, c['w'], c['u'], c['norms'], c['eps'], c['nvec'], c['vpc'], pd,
                                   pd if c['same'] else qd, 0.0, None, pq, ws, 4096, c['strides'])
        assert status == BADARG and L.emg3d_last_error(), change
        torch.cuda.synchronize()
        assert np.all(np.isnan(qd.cpu().numpy())) and np.all(np.isnan(pq.cpu().numpy())), change
    # the thresholds are not looked at when all norms are 2 and nothing is linearised
    assert _weighted_raw(h, ALPHA, None, w3, None, NORMS[0], (nan, -1.0), 6, 3, pd, qd, 0.0, None, pq, ws, 4096) == 0
    hd = [_padded(x) for x in h]
    wd, ud = _rows(w3, ncell), _rows(u3, ncell)
    diag = torch.full((3 * ncell,), nan, dtype=torch.float64, device=_dev())
    base = dict(vpc=3, norms=(1.0, 0.5, 1.0, 1.0), eps=(1e-3, 1e-3), u=_ptr(ud[0]), ws_=wd[1], us_=ud[1], out=_ptr(diag))
    for change in (dict(vpc=4), dict(vpc=0), dict(norms=(1.0, 0.5, 2.1, 1.0)), dict(u=None), dict(eps=(1e-3, 0.0)),
                   dict(ws_=ncell - 1), dict(us_=2), dict(out=None)):
        c = dict(base, **change)
        status = L.emg3d_dev_model_regulariser_weighted_diagonal(
            *shape, _ptr(hd[0]), _ptr(hd[1]), _ptr(hd[2]), *ALPHA, None, _ptr(wd[0]), c['ws_'], c['u'], c['us_'], *c['norms'],
            *c['eps'], c['vpc'], c['out'], _stream())
        assert status == BADARG and L.emg3d_last_error(), change
    torch.cuda.synchronize()
    assert np.all(np.isnan(diag.cpu().numpy()))
    # the _rd entries: a stride that is neither 0 nor >= n_cells
    t = torch.full((6 * ncell,), nan, dtype=torch.float64, device=_dev())
    table = _up(np.zeros((2, 8)))
    assert L.emg3d_dev_pcg_update_rd(ncell, 3, 2, 1, _ptr(t), _ptr(t), _ptr(t), _ptr(t), _ptr(t), _ptr(t), ncell - 1, None,
                                     _ptr(table), _ptr(pq), _ptr(ws), 4096, _stream()) == BADARG
    assert L.emg3d_dev_pcg_direction_rd(ncell, 3, 2, 1, _ptr(t), _ptr(t), _ptr(t), _ptr(t), ncell - 1, None, _ptr(table),
                                        _stream()) == BADARG
    torch.cuda.synchronize()
    assert np.all(np.isnan(t.cpu().numpy())) and np.all(table.cpu().numpy() == 0)


# ------------------------------------------------------------------ methods on the gpu ---
L1 = dict(norms=(1.0, 1.0, 1.0, 1.0), irls_eps=(1e-2, 1e-3))


class _Recorder:
    """The library with the names of the C functions that are looked up."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


@functools.lru_cache(maxsize=None)
def _weighted_dense(name):
    """Per case, once, on the instance and the right-hand sides of ``_dense`` of ``test_gauss_newton_solve``: strictly
    positive weights and a linearisation vector per component, a mask, dense H (``hessian_vec_block`` on the identity) and
    the weighted R (``regulariser_vec_block`` on the identity, checked against the ``longdouble`` operator of this file),
    three dampings over two decades around trace(H) / trace(R) (the iterations grow as the damping falls, and with them
    the time of the test) and per damping A, x*, cond_2(A) and the iterations of the dense reference's own CG with the
    Jacobi preconditioner and without."""
    import torch
    grid, rec, _, _, _, b, _ = _dense(name)
    n, ncell, shape = gradient._NCOMP[rec.model.case], grid.n_cells, tuple(grid.shape_cells)
    N = n * ncell
    rng = np.random.default_rng(23)
    active = rng.uniform(size=shape) < 0.85
    w = rng.uniform(0.2, 5.0, (n,) + shape)
    u = rng.standard_normal((n,) + shape)
    kw = dict(cell_weights=w, linearise_at=u if n > 1 else u[0], active=active, **L1, **REG)
    eye = torch.eye(N, dtype=torch.float64, device=_dev()).view(N, n, ncell)
    H = np.concatenate([_columns(rec.hessian_vec_block(eye[c:c + KC].contiguous(), columns_per_pass=KC))
                        for c in range(0, N, KC)]).T
    out = rec.regulariser_vec_block(eye, **kw)
    assert isinstance(out, torch.Tensor)                   # a device block in gives a device block out
    R = _columns(out).T
    unit = np.eye(ncell).reshape((ncell,) + shape, order='F')
    alphas = (REG['smallness'],) + REG['smoothness']
    for k in range(n):
        want, mag = (_flat(a).T for a in weighted_component_numpy(grid.h, alphas, active, w[k], u[k], L1['norms'],
                                                                  L1['irls_eps'], unit))
        blk = R[k * ncell:(k + 1) * ncell, k * ncell:(k + 1) * ncell]
        assert np.all(np.abs(blk - want) <= slack(L1['norms']) * EPS * mag)
        assert k == 0 or not np.array_equal(blk, R[:ncell, :ncell])
    assert np.count_nonzero(R) == sum(np.count_nonzero(R[k * ncell:(k + 1) * ncell, k * ncell:(k + 1) * ncell]) for k in range(n))
    assert np.array_equal(R, R.T)
    act = np.tile(active.ravel(order='F'), n)
    lams = np.trace(H[act][:, act]) / np.trace(R) * np.array([1e-1, 1.0, 1e1])
    dense = []
    for lam, bk in zip(lams, b):
        A = (H + lam * R)[act][:, act]
        ev = np.linalg.eigvalsh((A + A.T) / 2)
        its = [_pcg_numpy(A, bk[act], d, TOL, 20000) for d in (np.diagonal(A).copy(), np.ones(len(A)))]
        dense.append((A, np.linalg.solve(A, bk[act]), float(ev[-1] / ev[0]), its))
    return grid, rec, kw, act, lams, b, dense


def _check(tag, dense, x, info, act, b):
    """All states 1; the true residual ``|b - (H + lambda R) x| <= 2 tol |b|`` with the dense matrices; ``|x - x*| <=
    cond_2 2 tol |x*|``; entries outside ``active`` exactly 0."""
    assert np.all(info['state'] == 1), (tag, info)
    assert np.all(x[:, ~act] == 0.0)
    for k, (A, xs, cond, its) in enumerate(dense):
        res = np.linalg.norm(b[k][act] - A @ x[k][act]) / np.linalg.norm(b[k][act])
        err = np.linalg.norm(x[k][act] - xs) / np.linalg.norm(xs)
        record(f"weighted gauss_newton_solve {tag} column {k}: iterations {info['iterations'][k]} (dense CG {its}), true "
               f"residual / (2 tol) = {res / (2 * TOL):.2e}, error / (cond 2 tol) = {err / (cond * 2 * TOL):.2e}, "
               f"cond = {cond:.2e}")
        assert res <= 2 * TOL
        assert err <= cond * 2 * TOL


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['isotropic', 'triaxial'])
def test_weighted_solve_vs_dense(name):
    """Strictly positive weights, norms (1, 1, 1, 1), a mask, three dampings: with the Jacobi preconditioner (its diagonal
    of R per component) and without; the result does not depend on ``check_every``, bit for bit."""
    grid, rec, kw, act, lams, b, dense = _weighted_dense(name)
    before = dict(rec.n_solves)
    rhs = _to_model(rec, grid, b)
    for precondition in (True, False):
        maxit = 2 * max(d[3][0 if precondition else 1] for d in dense) + 10      # the dense CG converges within half of it
        x, info = rec.gauss_newton_solve(rhs, lams, tol=TOL, maxit=maxit, precondition=precondition, **kw)
        _check(f"{name} precondition={precondition}", dense, _from_model(x), info, act, b)
        if precondition:                                        # (x: with the default, a look every 4 iterations)
            y, other = rec.gauss_newton_solve(rhs, lams, tol=TOL, maxit=maxit, check_every=1, **kw)
            assert np.array_equal(x, y) and np.array_equal(info['iterations'], other['iterations'])
    assert rec.n_solves == before


@pytest.mark.gpu
def test_methods_routes_and_layouts(monkeypatch):
    """All new arguments ``None``: the entry points and the bits of a call without them; otherwise the weighted entries
    and the ``_rd`` kernels. Weights shaped like the cells are those of every component; device tensors give what NumPy
    gives; ``regulariser_vec_block`` returns NumPy for NumPy."""
    grid, rec, kw, act, lams, b, dense = _weighted_dense('triaxial')
    rhs = _to_model(rec, grid, b)
    none = dict(cell_weights=None, norms=None, linearise_at=None, irls_eps=None)
    proxy = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: proxy)
    x0, i0 = rec.gauss_newton_solve(rhs, lams, tol=1e-6, **REG)
    r0 = rec.regulariser_vec_block(rhs, **REG)
    def solver_calls():
        calls = [name for name in proxy.names if 'regulariser' in name or 'pcg' in name]
        del proxy.names[:]
        return calls
    plain = solver_calls()
    x1, i1 = rec.gauss_newton_solve(rhs, lams, tol=1e-6, **none, **REG)
    r1 = rec.regulariser_vec_block(rhs, **none, **REG)
    assert solver_calls() == plain and not any('weighted' in name or name.endswith('_rd') for name in plain)
    assert {'emg3d_dev_model_regulariser', 'emg3d_dev_model_regulariser_diagonal', 'emg3d_dev_pcg_update',
            'emg3d_dev_pcg_direction'} <= set(plain)
    assert np.array_equal(x0, x1) and np.array_equal(i0['iterations'], i1['iterations']) and np.array_equal(r0, r1)
    x2, i2 = rec.gauss_newton_solve(rhs, lams, tol=1e-6, **kw)
    weighted = set(solver_calls())
    assert {'emg3d_dev_model_regulariser_weighted', 'emg3d_dev_model_regulariser_weighted_diagonal', 'emg3d_dev_pcg_update_rd',
            'emg3d_dev_pcg_direction_rd'} <= weighted
    assert not {'emg3d_dev_model_regulariser', 'emg3d_dev_model_regulariser_diagonal', 'emg3d_dev_pcg_update',
                'emg3d_dev_pcg_direction'} & weighted
    monkeypatch.undo()
    # norms of 2 with weights of exactly 1, per component: the bits of the plain operator, through the weighted entries
    ones = np.ones((3,) + tuple(grid.shape_cells))
    assert np.array_equal(rec.regulariser_vec_block(rhs, cell_weights=ones, norms=(2, 2, 2, 2), **REG), r0)
    # one array of weights for all components = the same array per component; device tensors = NumPy
    w, u = kw['cell_weights'], kw['linearise_at']
    shared = dict(kw, cell_weights=w[0])
    a = rec.regulariser_vec_block(rhs, **shared)
    assert isinstance(a, np.ndarray) and a.shape == rhs.shape
    assert np.array_equal(a, rec.regulariser_vec_block(rhs, **dict(kw, cell_weights=np.stack([w[0]] * 3))))
    wd = _up(np.stack([c.ravel(order='F') for c in w]))
    ud = _up(np.stack([c.ravel(order='F') for c in u]))
    full = rec.regulariser_vec_block(rhs, **kw)
    assert np.array_equal(full, rec.regulariser_vec_block(rhs, **dict(kw, cell_weights=wd, linearise_at=ud)))
    assert np.array_equal(a, rec.regulariser_vec_block(rhs, **dict(kw, cell_weights=wd[0].contiguous(), linearise_at=ud)))
    want, mag = weighted_numpy(grid.h, (REG['smallness'],) + REG['smoothness'], kw['active'], w, u, L1['norms'],
                               L1['irls_eps'], rhs.reshape((-1,) + rhs.shape[-3:]), 3)
    assert np.all(np.abs(full.reshape(want.shape) - want) <= slack(L1['norms']) * EPS * mag)
    xd, idv = rec.gauss_newton_solve(rec.to_device(rhs), lams, tol=1e-6, **dict(kw, cell_weights=wd, linearise_at=ud))
    assert np.array_equal(rec.from_device(xd), x2) and np.array_equal(idv['iterations'], i2['iterations'])
