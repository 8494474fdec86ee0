"""The inner linear solve of a Gauss-Newton step: the kernels of ``csrc/regularise.h`` --
``emg3d_dev_model_regulariser``, ``emg3d_dev_model_regulariser_diagonal``, ``emg3d_dev_pcg_update`` / ``_scalar`` /
``_direction`` -- against NumPy in ``longdouble`` written out in this file, and
``ReciprocalSensitivity.regulariser_vec_block`` / ``gauss_newton_solve`` against dense matrices.

Inputs, the small survey and the recorder come from ``test_sensitivity``, the device helpers from ``test_reciprocal``;
figures that the GPU tests observe are printed and, with ``EMG3D_AMD_PARITY_FILE`` set, appended to that file.
"""
import functools
import itertools

import numpy as np
import pytest

from emg3d_amd import _lib, gradient
from test_reciprocal import _dev, _up
from test_sensitivity import EPS, FREQS, OPTS, RECS, SRCS, record, small_model

SYMBOLS = ('emg3d_model_regulariser_ws_len', 'emg3d_dev_model_regulariser', 'emg3d_dev_model_regulariser_diagonal',
           'emg3d_pcg_table_len', 'emg3d_pcg_ws_len', 'emg3d_dev_pcg_update', 'emg3d_dev_pcg_scalar',
           'emg3d_dev_pcg_direction')
LD = np.longdouble
ZERO = {'forward': 0, 'receiver': 0, 'jvec': 0, 'jtvec': 0}


# ----------------------------------------------------------------------- not gpu tests ---
def test_symbols_are_declared():
    header = open(_lib.HEADER).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name) and name + '(' in header
    assert any(s.endswith('regularise.h') for s in _lib.SOURCES)
    assert _lib.lib().emg3d_pcg_table_len(3) == 24


def test_methods_exist():
    for name in ('regulariser_vec_block', 'gauss_newton_solve'):
        assert callable(getattr(gradient.ReciprocalSensitivity, name))


def _bad_calls(shape):
    one = np.ones(shape)
    return [
        (dict(dampings=[]), "`dampings` must be a 1-D"), (dict(dampings=[1.0, 0.0]), "`dampings` must be a 1-D"),
        (dict(dampings=[-1.0]), "`dampings` must be a 1-D"), (dict(dampings=[np.nan]), "`dampings` must be a 1-D"),
        (dict(dampings=[[1.0]]), "`dampings` must be a 1-D"), (dict(dampings=2.0), "`dampings` must be a 1-D"),
        (dict(smoothness=(1.0, 1.0)), "`smoothness` must be three"),
        (dict(smoothness=(1.0, -1.0, 1.0)), "`smoothness` must be three"),
        (dict(smoothness=1.0), "`smoothness` must be three"), (dict(smallness=-1e-3), "`smallness` must be"),
        (dict(smallness=0.0, smoothness=(0.0, 0.0, 0.0)), "must not all be zero"),
        (dict(active=np.ones(shape)), "`active` must be a bool array"),
        (dict(active=np.ones(shape[:2], dtype=bool)), "`active` must be a bool array"),
        (dict(tol=0.0), "`tol` must be"), (dict(tol=1.0), "`tol` must be"), (dict(tol=-1e-3), "`tol` must be"),
        (dict(maxit=0), "`maxit` must be an integer >= 1"), (dict(maxit=2.5), "`maxit` must be an integer >= 1"),
        (dict(check_every=0), "`check_every` must be an integer >= 1"),
        (dict(check_every=True), "`check_every` must be an integer >= 1"),
        (dict(rhs=np.stack([one, one])), "`rhs` must be one model-shaped vector or a block of K"),
        (dict(rhs=np.ones((3, 3))), "`rhs` must be real with shape"), (dict(columns_per_pass=0), "`columns_per_pass`"),
        (dict(weights={('a', 'f'): np.ones(2)}), "one value per receiver"),
    ]


def test_arguments_are_validated_before_any_gpu_work():
    """Every message of the validation, with "Provided:", without a device; ``n_solves`` and ``kept_bytes`` stay."""
    grid, model = small_model()
    shape = tuple(grid.shape_cells)
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    for kwargs, match in _bad_calls(shape):
        args = dict(rhs=np.ones(shape), dampings=[1.0, 10.0, 100.0])
        args.update(kwargs)
        with pytest.raises(ValueError, match=match) as err:
            rec.gauss_newton_solve(**args)
        assert "Provided:" in str(err.value), kwargs
    for kwargs, match in ((dict(smoothness=(1.0, 1.0)), "`smoothness`"), (dict(smallness=-1.0), "`smallness`"),
                          (dict(smallness=0.0, smoothness=(0, 0, 0)), "must not all be zero"),
                          (dict(active=np.ones(shape)), "`active`"), (dict(vectors=np.ones(shape[:2])), "`vectors`")):
        args = dict(vectors=np.ones((2,) + shape))
        args.update(kwargs)
        with pytest.raises(ValueError, match=match) as err:
            rec.regulariser_vec_block(**args)
        assert "Provided:" in str(err.value), kwargs
    assert rec.n_solves == ZERO and rec.kept_bytes == 0


def test_precondition_needs_the_model_grid_as_hessian_diagonal():
    from test_reciprocal import _comp_grid
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, grids=_comp_grid())
    with pytest.raises(NotImplementedError) as a:
        rec.hessian_diagonal()
    with pytest.raises(NotImplementedError) as b:
        rec.gauss_newton_solve(np.ones(grid.shape_cells), [1.0])
    assert str(a.value).split(':', 1)[1] == str(b.value).split(':', 1)[1]
    assert rec.n_solves == ZERO and rec.kept_bytes == 0


def test_no_cpu_fallback_without_gpu():
    if _lib.lib().emg3d_device_count() > 0:
        pytest.skip("GPU present")
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.regulariser_vec_block(np.ones((1,) + tuple(grid.shape_cells)))
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.gauss_newton_solve(np.ones(grid.shape_cells), [1.0, 2.0])
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.gauss_newton_solve(np.ones(grid.shape_cells), [1.0], precondition=False)


# ------------------------------------------------------------------------ the checker ---
def regulariser_numpy(h, alphas, mask, v):
    """``R v`` in ``longdouble`` for v (nvec, nx, ny, nz), and the sum of the magnitudes of its terms: (alpha_s V |v|
    and, per kept face, coefficient x (|v[c]| + |v[c']|)); h: three width arrays, mask: bool (nx, ny, nz) or None."""
    hx, hy, hz = (np.asarray(w, dtype=LD) for w in h)
    nx, ny, nz = len(hx), len(hy), len(hz)
    a = np.ones((nx, ny, nz), dtype=LD) if mask is None else mask.astype(LD)
    v = np.asarray(v, dtype=LD)
    vol = hx[:, None, None] * hy[None, :, None] * hz[None, None, :]
    out, mag = LD(alphas[0]) * vol * v, LD(alphas[0]) * vol * np.abs(v)
    area = (hy[None, :, None] * hz[None, None, :], hx[:, None, None] * hz[None, None, :], hx[:, None, None] * hy[None, :, None])
    for d, w in enumerate((hx, hy, hz)):
        if len(w) < 2:
            continue
        lo = tuple(slice(0, -1) if k == d else slice(None) for k in range(3))
        hi = tuple(slice(1, None) if k == d else slice(None) for k in range(3))
        dist = (0.5 * (w[:-1] + w[1:])).reshape([-1 if k == d else 1 for k in range(3)])
        coef = LD(alphas[1 + d]) * area[d] / dist * a[lo] * a[hi]
        vlo, vhi = v[(slice(None),) + lo], v[(slice(None),) + hi]
        out[(slice(None),) + lo] += coef * (vlo - vhi)
        out[(slice(None),) + hi] += coef * (vhi - vlo)
        mag[(slice(None),) + lo] += coef * (np.abs(vlo) + np.abs(vhi))
        mag[(slice(None),) + hi] += coef * (np.abs(vlo) + np.abs(vhi))
    return out * a, mag * a


def _flat(v):
    """(nvec, nx, ny, nz) -> (nvec, n_cells), cells x fastest."""
    return np.stack([c.ravel(order='F') for c in v])


def _padded(a, pad=5, dtype=float):
    """``a`` flattened, followed by NaN that must never be read."""
    a = np.asarray(a, dtype=dtype).ravel()
    return _up(np.concatenate([a, np.full(pad, np.nan, dtype=dtype)]))


def _regulariser(h, alphas, mask, p, q0, beta, lam, vpc, with_pq=True):
    """The kernel on p (nvec, nx, ny, nz): (q (nvec, n_cells), pq (ncol,) or None); every buffer NaN behind its end."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    nx, ny, nz = (len(w) for w in h)
    nvec, ncell, ncol = len(p), nx * ny * nz, len(p) // vpc
    hd = [_padded(w) for w in h]
    md = None if mask is None else _up(np.concatenate([mask.ravel(order='F').astype(np.uint8), np.full(7, 1, np.uint8)]))
    pd = _padded(_flat(p))
    qd = _padded(np.full((nvec, ncell), np.nan) if q0 is None else q0)
    ld = None if lam is None else _padded(lam)
    ws_len = L.emg3d_model_regulariser_ws_len(nx, ny, nz, nvec, vpc)
    assert ws_len > 0
    ws = torch.full((ws_len,), float('nan'), dtype=torch.float64, device=_dev())
    pq = torch.full((ncol + 2,), float('nan'), dtype=torch.float64, device=_dev())
    _lib.check(L.emg3d_dev_model_regulariser(
        nx, ny, nz, _ptr(hd[0]), _ptr(hd[1]), _ptr(hd[2]), *[float(a) for a in alphas], None if md is None else _ptr(md),
        nvec, vpc, _ptr(pd), _ptr(qd), float(beta), None if ld is None else _ptr(ld), _ptr(pq) if with_pq else None,
        _ptr(ws) if with_pq else None, ws_len if with_pq else 0, _stream()), 'emg3d_dev_model_regulariser')
    q = qd.cpu().numpy()
    assert np.all(np.isnan(q[nvec * ncell:])) and np.all(np.isnan(pq.cpu().numpy()[ncol:]))     # nothing behind the end
    return q[:nvec * ncell].reshape(nvec, ncell), (pq.cpu().numpy()[:ncol] if with_pq else None)


def _widths(n, first, rng):
    """n non-uniform widths, stretched by 1.3 from a random start."""
    return first * 1.3 ** np.arange(n) * rng.uniform(0.9, 1.1, n)


ALPHAS = [(2e-3, 0.0, 0.0, 0.0), (0.0, 1.5, 0.0, 0.0), (0.0, 0.0, 0.7, 0.0), (0.0, 0.0, 0.0, 2.0), (1e-3, 1.0, 0.5, 2.0)]
VECTORS = [(1, 1), (3, 1), (3, 3), (9, 1), (9, 3)]       # (nvec, vec_per_col): nvec is a multiple of vec_per_col


def _masks(rng, shape):
    plane = np.ones(shape, dtype=bool)
    plane[:, :, shape[2] // 2] = False                      # one whole inactive plane (nz = 1: every cell)
    return [None, rng.uniform(size=shape) < 0.7, plane]


# ------------------------------------------------------------------ kernels on the gpu ---
@pytest.mark.gpu
@pytest.mark.parametrize('ny, nz', [(1, 1), (2, 5), (5, 2)])
@pytest.mark.parametrize('nx', [1, 2, 63, 64, 65, 130])
def test_regulariser_vs_numpy(nx, ny, nz):
    """Per output ``|got - want| <= 16 eps (|beta q| + |lam| sum |terms of R p|)``: the seven terms are added one after
    the other (7 roundings of a partial sum), a coefficient carries 4 roundings, the difference of two values, the
    product with lambda and the final sum one each -- 14 half-eps in all. Per column ``|<p,q> - want| <= (N + 16) eps
    sum |p| |q|``, N the elements of a column: the worst case of any order of summation. All combinations of the vector
    layouts, beta, lambda, the masks and the coefficient sets; every buffer is followed by NaN."""
    rng = np.random.default_rng(1000 * nx + 10 * ny + nz)
    h = [_widths(nx, 40.0, rng), _widths(ny, 55.0, rng), _widths(nz, 25.0, rng)]
    shape, ncell = (nx, ny, nz), nx * ny * nz
    worst_q = worst_pq = 0.0
    for (nvec, vpc), mask, alphas, beta, use_lam in itertools.product(VECTORS, _masks(rng, shape), ALPHAS, (0.0, 1.0),
                                                                       (False, True)):
        ncol = nvec // vpc
        p = rng.standard_normal((nvec,) + shape)
        q0 = rng.standard_normal((nvec, ncell)) if beta else None
        lam = 10 ** rng.uniform(-2, 2, ncol) if use_lam else None
        got, pq = _regulariser(h, alphas, mask, p, q0, beta, lam, vpc)
        rp, mag = regulariser_numpy(h, alphas, mask, p)
        lcol = np.repeat(np.ones(ncol) if lam is None else lam, vpc).astype(LD)[:, None]
        want = lcol * _flat(rp) + (beta * q0.astype(LD) if beta else 0)
        bound = 16 * EPS * (lcol * _flat(mag) + (np.abs(beta * q0) if beta else 0))
        assert not np.any(np.isnan(got))
        err = np.abs(got - want)
        assert np.all(err <= bound), (nvec, vpc, alphas, beta, use_lam)
        if mask is not None and not beta:
            assert np.all(got[:, ~mask.ravel(order='F')] == 0.0)          # rows of inactive cells: exactly 0
        worst_q = max(worst_q, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
        pf = _flat(p).astype(LD)
        want_pq = np.sum((pf * got.astype(LD)).reshape(ncol, -1), axis=1)
        bound_pq = (vpc * ncell + 16) * EPS * np.sum(np.abs(pf * got).reshape(ncol, -1), axis=1)
        assert np.all(np.abs(pq - want_pq) <= bound_pq), (nvec, vpc, alphas, beta, use_lam)
        some = bound_pq > 0
        worst_pq = max(worst_pq, float(np.max(np.abs(pq - want_pq)[some] / bound_pq[some], initial=0.0)))
    # without pq no workspace is needed, and the vectors are the same bits; twice: the same bits
    again = [_regulariser(h, ALPHAS[-1], mask, p, q0, beta, lam, vpc, with_pq=w) for w in (False, True, True)]
    assert np.array_equal(again[0][0], again[1][0]) and np.array_equal(again[1][0], again[2][0])
    assert np.array_equal(again[1][1], again[2][1])
    record(f"regulariser {nx} x {ny} x {nz}: max |diff| / bound = {worst_q:.2e} (16 eps sum |terms|), "
           f"<p,q> {worst_pq:.2e} ((N + 16) eps)")


@pytest.mark.gpu
def test_regulariser_properties():
    """Constants: the roughness part vanishes exactly, ``R c = alpha_s V c`` within 16 eps of that one product. Symmetry:
    every output is within 16 eps of the sum of the magnitudes of its terms (the test above), the exact operator is
    symmetric, hence ``|<u, R v> - <R u, v>| <= 16 eps (sum |u| mag(v) + sum |v| mag(u))``; ``<v, R v> >= 0`` as the
    kernel itself sums it; rows AND columns of inactive cells are exactly 0."""
    rng = np.random.default_rng(7)
    shape = (67, 5, 3)
    h = [_widths(n, 30.0, rng) for n in shape]
    mask = rng.uniform(size=shape) < 0.8
    vol = (h[0][:, None, None] * h[1][None, :, None] * h[2][None, None, :])
    for m in (None, mask):
        const = np.full((1,) + shape, -3.7)
        got, _ = _regulariser(h, (0.0, 1.0, 2.0, 3.0), m, const, None, 0.0, None, 1)
        assert np.all(got == 0.0)                                                 # exactly annihilated
        got, _ = _regulariser(h, ALPHAS[-1], m, const, None, 0.0, None, 1)
        want = (ALPHAS[-1][0] * vol * const[0] * (1 if m is None else m)).ravel(order='F')
        assert np.all(np.abs(got[0] - want) <= 16 * EPS * np.abs(want))
        u, v = rng.standard_normal((2, 1) + shape)
        (ru, uru), (rv, vrv) = (_regulariser(h, ALPHAS[-1], m, w, None, 0.0, None, 1) for w in (u, v))
        mu, mv = (_flat(regulariser_numpy(h, ALPHAS[-1], m, w)[1]) for w in (u, v))
        uf, vf = _flat(u).astype(LD), _flat(v).astype(LD)
        asym = abs(float(np.sum(uf * rv) - np.sum(ru * vf)))
        bound = float(16 * EPS * (np.sum(np.abs(uf) * mv) + np.sum(np.abs(vf) * mu)))
        record(f"regulariser symmetry (mask: {m is not None}): |<u,Rv> - <Ru,v>| / bound = {asym / bound:.2e}")
        assert asym <= bound
        assert uru[0] >= 0 and vrv[0] >= 0
    # rows: inactive outputs are 0 even where p is NaN there; columns: what an inactive cell holds changes nothing
    dirty = v.copy()
    dirty[0][~mask] = np.nan
    clean = np.where(mask, v, 0.0)
    a, _ = _regulariser(h, ALPHAS[-1], mask, dirty, None, 0.0, None, 1, with_pq=False)
    b, _ = _regulariser(h, ALPHAS[-1], mask, clean, None, 0.0, None, 1, with_pq=False)
    assert np.array_equal(a, b) and np.all(a[0][~mask.ravel(order='F')] == 0.0)


def _diagonal(h, alphas, mask):
    import torch
    from emg3d_amd._device import _ptr, _stream
    nx, ny, nz = (len(w) for w in h)
    hd = [_padded(w) for w in h]
    md = None if mask is None else _up(mask.ravel(order='F').astype(np.uint8))
    out = torch.full((nx * ny * nz + 3,), float('nan'), dtype=torch.float64, device=_dev())
    _lib.check(_lib.lib().emg3d_dev_model_regulariser_diagonal(
        nx, ny, nz, _ptr(hd[0]), _ptr(hd[1]), _ptr(hd[2]), *[float(a) for a in alphas], None if md is None else _ptr(md),
        _ptr(out), _stream()), 'emg3d_dev_model_regulariser_diagonal')
    out = out.cpu().numpy()
    assert np.all(np.isnan(out[nx * ny * nz:])) and not np.any(np.isnan(out[:nx * ny * nz]))
    return out[:nx * ny * nz]


@pytest.mark.gpu
def test_regulariser_diagonal_vs_unit_vectors():
    """3 x 2 x 2 cells: the diagonal kernel against ``R`` applied to the twelve unit vectors, within 16 eps of the sum of
    the magnitudes of the terms (of the kernel and of the checker); with a mask: 0 on inactive cells."""
    rng = np.random.default_rng(11)
    shape = (3, 2, 2)
    h = [_widths(n, 20.0, rng) for n in shape]
    mask = np.ones(shape, dtype=bool)
    mask[1, 0, 1] = mask[2, 1, 0] = False
    eye = np.eye(12).reshape((12,) + shape, order='F')
    for m in (None, mask):
        got = _diagonal(h, ALPHAS[-1], m)
        dense, _ = _regulariser(h, ALPHAS[-1], m, eye, None, 0.0, None, 1, with_pq=False)
        want, mag = regulariser_numpy(h, ALPHAS[-1], m, eye)
        want, mag = np.diagonal(_flat(want)), np.diagonal(_flat(mag))
        assert np.all(np.abs(got - want) <= 16 * EPS * mag) and np.all(np.abs(got - np.diagonal(dense)) <= 32 * EPS * mag)
        assert np.array_equal(dense, dense.T)                      # the same coefficient from either side of a face
        if m is not None:
            assert np.all(got[~m.ravel(order='F')] == 0.0)


def _pcg(ncell, vpc, K, first, x, r, p, q, hd, rd, mask, table, pq, tol, direction=True):
    """update -> scalar -> direction on copies of the host arrays; returns (x, r, p, table) as NumPy."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    xd, rdv, pd, qd = (_padded(a) for a in (x, r, p, q))
    hdd, rdd = (None if a is None else _padded(a) for a in (hd, rd))
    md = None if mask is None else _up(mask.astype(np.uint8))
    td, pqd = _up(table), _padded(pq)
    ws_len = L.emg3d_pcg_ws_len(ncell, K)
    ws = torch.full((ws_len,), float('nan'), dtype=torch.float64, device=_dev())
    opt = [None if t is None else _ptr(t) for t in (hdd, rdd, md)]
    _lib.check(L.emg3d_dev_pcg_update(ncell, vpc, K, first, _ptr(xd), _ptr(rdv), _ptr(pd), _ptr(qd), *opt, _ptr(td), _ptr(pqd),
                                      _ptr(ws), ws_len, _stream()), 'emg3d_dev_pcg_update')
    _lib.check(L.emg3d_dev_pcg_scalar(ncell, K, first, tol, _ptr(td), _ptr(pqd), _ptr(ws), ws_len, _stream()),
               'emg3d_dev_pcg_scalar')
    if direction:
        _lib.check(L.emg3d_dev_pcg_direction(ncell, vpc, K, first, _ptr(pd), _ptr(rdv), *opt, _ptr(td), _stream()),
                   'emg3d_dev_pcg_direction')
    n = K * vpc * ncell
    return xd.cpu().numpy()[:n], rdv.cpu().numpy()[:n], pd.cpu().numpy()[:n], td.cpu().numpy()


def _z_numpy(r, act, hd, rd, lam):
    """M r in longdouble for one column (vpc, ncell)."""
    if hd is None:
        return np.where(act, r, 0).astype(LD)
    d = hd.astype(LD) + LD(lam) * rd.astype(LD)[None]
    return np.where(act, r.astype(LD) / d, 0)


@pytest.mark.gpu
@pytest.mark.parametrize('jacobi', [True, False])
@pytest.mark.parametrize('K', [1, 3, 9])
@pytest.mark.parametrize('ncell', [1, 257, 8197, 3 * 8192 + 1])
def test_pcg_kernels_vs_numpy(ncell, K, jacobi):
    """One iteration of the three kernels against NumPy with the table's own scalars. Elements: 4 eps of the magnitudes
    (alpha p or alpha q: 2 roundings, the sum 1; z: 3). Sums: ``(N + 16) eps sum |r| |z|``. Column 1 is frozen (K >= 3):
    x, r, p keep their bits; column 2 has <p,q> <= 0 -> state 2; column 3 (K = 9) a NaN -> state 3, column 4 an inf:
    neither puts a NaN into x. The same call twice: the same bits."""
    rng = np.random.default_rng(ncell + 7 * K + jacobi)
    vpc = 2 if K == 3 else 1
    N = vpc * ncell
    x, r, p, q = rng.standard_normal((4, K, vpc, ncell))
    hd, rd = (rng.uniform(0.5, 2.0, (vpc, ncell)), rng.uniform(0.1, 1.0, ncell)) if jacobi else (None, None)
    act = rng.uniform(size=ncell) < 0.8 if ncell > 1 else np.array([True])
    table = np.zeros((K, 8))
    table[:, 0] = 10 ** rng.uniform(-1, 1, K)
    table[:, 1] = 10 ** rng.uniform(0, 8, K) * N            # <b,b>: some columns converge, some do not
    table[:, 2] = rng.uniform(0.5, 2.0, K)
    table[:, 6] = 4
    pq = rng.uniform(0.5, 2.0, K) * 50
    tol = 1e-3
    if K >= 3:
        table[1, 7] = 1.0
        pq[2] = -0.25
    if K == 9:
        pq[3], pq[4] = np.nan, np.inf
        q[3, 0, 0] = np.nan
    got = _pcg(ncell, vpc, K, 0, x, r, p, q, hd, rd, act, table, pq, tol)
    gx, gr, gp = (a.reshape(K, vpc, ncell) for a in got[:3])
    gt = got[3]
    assert not np.any(np.isnan(gx))
    worst = 0.0
    for k in range(K):
        lam, rz0 = table[k, 0], table[k, 2]
        if (K >= 3 and k in (1, 2)) or (K == 9 and k in (3, 4)):
            assert np.array_equal(gx[k], x[k]) and np.array_equal(gr[k], r[k], equal_nan=True) and np.array_equal(gp[k], p[k])
            want_state = {1: 1, 2: 2, 3: 3, 4: 3}[k]
            assert gt[k, 7] == want_state and gt[k, 6] == 4 and gt[k, 2] == rz0
            if k != 1:
                assert gt[k, 4] == pq[k] or (np.isnan(pq[k]) and np.isnan(gt[k, 4]))
            continue
        alpha = rz0 / pq[k]
        assert np.all(np.abs(gx[k] - (x[k] + LD(alpha) * p[k])) <= 4 * EPS * (np.abs(x[k]) + np.abs(alpha * p[k])))
        want_r = np.where(act, r[k] - LD(alpha) * q[k], 0)
        assert np.all(np.abs(gr[k] - want_r) <= 4 * EPS * (np.abs(r[k]) + np.abs(alpha * q[k])))
        assert np.all(gr[k][:, ~act] == 0.0)
        z = _z_numpy(gr[k], act, hd, rd, lam)
        rz, rr = np.sum(gr[k] * z), np.sum(gr[k].astype(LD) ** 2)
        brz, brr = (N + 16) * EPS * np.sum(np.abs(gr[k] * z)), (N + 16) * EPS * rr
        assert abs(gt[k, 2] - rz) <= brz and abs(gt[k, 5] - rr) <= brr
        worst = max(worst, float(abs(gt[k, 2] - rz) / brz), float(abs(gt[k, 5] - rr) / brr))
        assert gt[k, 3] == rz0 and gt[k, 4] == pq[k] and gt[k, 6] == 5 and gt[k, 0] == lam and gt[k, 1] == table[k, 1]
        state = 1 if gt[k, 5] <= tol * tol * gt[k, 1] else 0                    # the table's own sums
        assert gt[k, 7] == state
        if state == 0:
            beta = gt[k, 2] / gt[k, 3]
            assert np.all(np.abs(gp[k] - (z + LD(beta) * p[k])) <= 4 * EPS * (np.abs(z) + np.abs(beta * p[k])))
        else:
            assert np.array_equal(gp[k], p[k])
    record(f"pcg kernels n={ncell} K={K} jacobi={jacobi}: sums max |diff| / bound = {worst:.2e} ((N + 16) eps)")
    again = _pcg(ncell, vpc, K, 0, x, r, p, q, hd, rd, act, table, pq, tol)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, again))
    # the set-up: r holds b, which is masked and summed; p = z; <b,b> = 0 -> state 1 at iteration 0
    b = r.copy()
    b[K - 1] = 0.0
    first = np.zeros((K, 8))
    first[:, 0] = table[:, 0]
    nan = np.full_like(x, np.nan)
    fx, fr, fp, ft = _pcg(ncell, vpc, K, 1, nan, b, nan, nan, hd, rd, act, first, np.full(K, np.nan), tol)
    fr, fp = fr.reshape(K, vpc, ncell), fp.reshape(K, vpc, ncell)
    for k in range(K):
        assert np.array_equal(fr[k], np.where(act, b[k], 0.0))
        z = _z_numpy(fr[k], act, hd, rd, first[k, 0])
        rr = np.sum(fr[k].astype(LD) ** 2)
        assert abs(ft[k, 5] - rr) <= (N + 16) * EPS * rr and ft[k, 1] == ft[k, 5] and ft[k, 6] == 0
        assert abs(ft[k, 2] - np.sum(fr[k] * z)) <= (N + 16) * EPS * np.sum(np.abs(fr[k] * z))
        if rr == 0:
            assert ft[k, 7] == 1 and np.all(np.isnan(fp[k]))                    # frozen at once: p is not touched
        else:
            assert ft[k, 7] == 0 and np.all(np.abs(fp[k] - z) <= 4 * EPS * np.abs(z))


# ------------------------------------------------------------------ methods on the gpu ---
CASES = {'isotropic': ('isotropic', 'Resistivity'), 'VTI': ('VTI', 'Conductivity'), 'triaxial': ('triaxial', 'Resistivity')}
REG = dict(smallness=1e-3, smoothness=(1.0, 0.5, 2.0))
TOL = 1e-10
KC = 8


def _survey(name, **kwargs):
    grid, model = small_model(*CASES[name])
    return grid, gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, solver_opts=OPTS, **kwargs)


def _columns(block):
    """Device block (K, n, n_cells) -> NumPy (K, n * n_cells)."""
    return block.reshape(len(block), -1).cpu().numpy()


def _pcg_numpy(A, b, d, tol, maxit=5000):
    """Textbook Jacobi-preconditioned CG on the dense system: the iterations to ``|r| <= tol |b|``."""
    x, r = np.zeros_like(b), b.copy()
    z = r / d
    p, rz = z.copy(), r @ z
    for it in range(1, maxit + 1):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        if np.linalg.norm(r) <= tol * np.linalg.norm(b):
            return it
        z = r / d
        rz, old = r @ z, rz
        p = z + rz / old * p
    raise AssertionError("the dense reference's own CG did not converge")


@functools.lru_cache(maxsize=None)
def _dense(name, masked=False):
    """Per case, once: the instance after ``forward()``, dense H (``hessian_vec_block`` on the identity in chunks of
    ``KC`` columns) and R (``regulariser_vec_block`` on the identity, checked against the NumPy operator), three dampings
    over four decades around trace(H) / trace(R), the right-hand sides, and per damping A, x* = solve(A, b), cond_2(A)
    and the iterations of the dense reference's own CG."""
    import torch
    grid, rec = _survey(name)
    rec.forward()
    n, ncell = gradient._NCOMP[rec.model.case], grid.n_cells
    N = n * ncell
    rng = np.random.default_rng(5)
    active = (rng.uniform(size=grid.shape_cells) < 0.85) if masked else None
    eye = torch.eye(N, dtype=torch.float64, device=_dev()).view(N, n, ncell)
    H = np.concatenate([_columns(rec.hessian_vec_block(eye[c:c + KC].contiguous(), columns_per_pass=KC))
                        for c in range(0, N, KC)]).T
    R = _columns(rec.regulariser_vec_block(eye, active=active, **REG)).T
    unit = np.eye(ncell).reshape((ncell,) + tuple(grid.shape_cells), order='F')
    alphas = (REG['smallness'],) + REG['smoothness']
    want, mag = (_flat(a).T for a in regulariser_numpy(grid.h, alphas, active, unit))
    assert np.all(np.abs(R[:ncell, :ncell] - want) <= 16 * EPS * mag)
    for k in range(1, n):                                  # every component on its own, the same operator
        assert np.array_equal(R[k * ncell:(k + 1) * ncell, k * ncell:(k + 1) * ncell], R[:ncell, :ncell])
    assert np.count_nonzero(R) == n * np.count_nonzero(R[:ncell, :ncell])
    act = np.ones(N, dtype=bool) if active is None else np.tile(active.ravel(order='F'), n)
    lam0 = np.trace(H[act][:, act]) / np.trace(R)
    lams = lam0 * np.array([1e-2, 1.0, 1e2])
    b = rng.standard_normal((3, N))
    out = []
    for lam, bk in zip(lams, b):
        A = (H + lam * R)[act][:, act]
        ev = np.linalg.eigvalsh((A + A.T) / 2)
        xs = np.linalg.solve(A, bk[act])
        its = _pcg_numpy(A, bk[act], np.diagonal(A).copy(), TOL)
        out.append((A, xs, float(ev[-1] / ev[0]), its))
    return grid, rec, active, act, lams, b, out


def _to_model(rec, grid, cols):
    """(K, n * n_cells) columns -> the NumPy block (K, n, nx, ny, nz) that the methods take."""
    n = gradient._NCOMP[rec.model.case]
    return np.stack([np.stack([c.reshape(grid.shape_cells, order='F') for c in col.reshape(n, -1)]) for col in cols])


def _from_model(x):
    """The NumPy result (K,) + the shape of ``jtvec`` -> (K, n * n_cells) columns."""
    K = len(x)
    x = x.reshape((K, -1) + x.shape[-3:])
    return np.stack([np.concatenate([c.ravel(order='F') for c in col]) for col in x])


def _check_solution(tag, dense, x, info, act, b, extra=0.0):
    """All states 1; true residual <= 2 tol |b| with the dense matrices; |x - x*| <= cond_2(A) 2 tol |x*| (+ extra |x*|):
    a relative residual rho bounds the relative error by cond rho."""
    assert np.all(info['state'] == 1), (tag, info)
    assert np.all(x[:, ~act] == 0.0)
    for k, (A, xs, cond, its) in enumerate(dense):
        res = np.linalg.norm(b[k][act] - A @ x[k][act]) / np.linalg.norm(b[k][act])
        err = np.linalg.norm(x[k][act] - xs) / np.linalg.norm(xs)
        record(f"gauss_newton_solve {tag} column {k}: iterations {info['iterations'][k]} (dense CG {its}), true residual "
               f"/ (2 tol) = {res / (2 * TOL):.2e}, error / (cond 2 tol) = {err / (cond * 2 * TOL + extra):.2e}, "
               f"cond = {cond:.2e}")
        assert res <= 2 * TOL
        assert err <= cond * 2 * TOL + extra


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_solve_vs_dense(name):
    grid, rec, active, act, lams, b, dense = _dense(name)
    before = dict(rec.n_solves)
    maxit = 2 * max(d[3] for d in dense) + 10          # the dense CG converges within half of it
    x, info = rec.gauss_newton_solve(_to_model(rec, grid, b), lams, tol=TOL, maxit=maxit, columns_per_pass=KC, **REG)
    n = gradient._NCOMP[rec.model.case]
    assert x.shape == (3,) + ((n,) if n > 1 else ()) + tuple(grid.shape_cells)
    _check_solution(name, dense, _from_model(x), info, act, b)
    assert info['hessian_passes'] >= info['iterations'].max() and len(info['history']) >= 2
    assert rec.n_solves == before


@pytest.mark.gpu
def test_columns_are_independent_and_one_rhs_is_a_block_of_copies():
    grid, rec, active, act, lams, b, dense = _dense('isotropic')
    maxit = 2 * max(d[3] for d in dense) + 10
    rhs = _to_model(rec, grid, b)
    together = _from_model(rec.gauss_newton_solve(rhs, lams, tol=TOL, maxit=maxit, **REG)[0])
    for k, (A, xs, cond, its) in enumerate(dense):
        alone, info = rec.gauss_newton_solve(rhs[k:k + 1], lams[k:k + 1], tol=TOL, maxit=maxit, **REG)
        assert info['state'][0] == 1
        diff = np.linalg.norm(_from_model(alone)[0] - together[k])
        assert diff <= 2 * cond * TOL * np.linalg.norm(xs)
    one, i1 = rec.gauss_newton_solve(rhs[0], lams, tol=TOL, maxit=maxit, **REG)
    copies, i2 = rec.gauss_newton_solve(np.stack([rhs[0]] * 3), lams, tol=TOL, maxit=maxit, **REG)
    assert np.array_equal(one, copies) and np.array_equal(i1['iterations'], i2['iterations'])
    assert one.shape == (3,) + tuple(grid.shape_cells)


@pytest.mark.gpu
def test_a_stopped_column_is_frozen():
    """Dampings [1e4 lambda, lambda]: the first column stops earlier; its x has the same bits with ``check_every`` 1
    and 3, and with ``maxit`` at its own count or larger."""
    grid, rec, active, act, lams, b, dense = _dense('isotropic')
    rhs = _to_model(rec, grid, b[:2])
    lam = np.array([1e4 * lams[1], lams[1]])
    maxit = 2 * dense[1][3] + 10                       # the dense CG of lams[1] converges within half of it, to 1e-10
    runs = [rec.gauss_newton_solve(rhs, lam, tol=1e-8, maxit=maxit, check_every=ce, **REG) for ce in (1, 3)]
    (x1, i1), (x3, i3) = runs
    assert np.all(i1['state'] == 1) and i1['iterations'][0] < i1['iterations'][1]
    assert np.array_equal(x1, x3) and np.array_equal(i1['iterations'], i3['iterations'])
    assert np.array_equal(i1['relative_residual'], i3['relative_residual'])
    short, ishort = rec.gauss_newton_solve(rhs, lam, tol=1e-8, maxit=int(i1['iterations'][0]), **REG)
    assert np.array_equal(short[0], x1[0]) and ishort['state'][0] == 1 and ishort['state'][1] == 0
    assert ishort['iterations'][1] == i1['iterations'][0]
    record(f"gauss_newton_solve freezing: iterations {i1['iterations'].tolist()}, passes {i1['hessian_passes']} / "
           f"{i3['hessian_passes']} with check_every 1 / 3")


@pytest.mark.gpu
def test_mask():
    grid, rec, active, act, lams, b, dense = _dense('isotropic', True)
    maxit = 2 * max(d[3] for d in dense) + 10
    x, info = rec.gauss_newton_solve(_to_model(rec, grid, b), lams, tol=TOL, maxit=maxit, active=active, **REG)
    assert np.all(x[:, ~active] == 0.0)
    _check_solution('masked', dense, _from_model(x), info, act, b)


@pytest.mark.gpu
def test_without_preconditioner_device_route_and_zero_rhs():
    grid, rec, active, act, lams, b, dense = _dense('isotropic')
    before = dict(rec.n_solves)
    maxit = 2 * max(d[3] for d in dense) + 10
    rhs = _to_model(rec, grid, b)
    x, info = rec.gauss_newton_solve(rhs, lams, tol=TOL, maxit=maxit, **REG)
    # no preconditioner: its own dense CG says how many iterations it may need
    plain = 2 * max(_pcg_numpy(A, bk[act], np.ones(len(A)), TOL, 20000) for (A, *_), bk in zip(dense, b)) + 10
    xn, infon = rec.gauss_newton_solve(rhs, lams, tol=TOL, maxit=plain, precondition=False, **REG)
    _check_solution('precondition=False', dense, _from_model(xn), infon, act, b)
    record(f"gauss_newton_solve iterations: Jacobi {info['iterations'].tolist()}, none {infon['iterations'].tolist()}")
    # rhs on the device: a device block with the bits of the NumPy route
    xd, infod = rec.gauss_newton_solve(rec.to_device(rhs), lams, tol=TOL, maxit=maxit, **REG)
    import torch
    assert isinstance(xd, torch.Tensor) and np.array_equal(rec.from_device(xd), x)
    assert np.array_equal(infod['iterations'], info['iterations'])
    host = rec.gauss_newton_solve(rec.to_device(rhs), lams, tol=TOL, maxit=maxit, on_device=False, **REG)[0]
    assert isinstance(host, np.ndarray) and np.array_equal(host, x)
    one = rec.gauss_newton_solve(rec.to_device(rhs)[0], lams, tol=TOL, maxit=maxit, **REG)[0]
    assert np.array_equal(rec.from_device(one), rec.gauss_newton_solve(rhs[0], lams, tol=TOL, maxit=maxit, **REG)[0])
    # rhs = 0: x = 0, state 1 at iteration 0, no pass
    x0, info0 = rec.gauss_newton_solve(np.zeros(grid.shape_cells), lams, tol=TOL, **REG)
    assert np.all(x0 == 0.0) and np.all(info0['state'] == 1) and np.all(info0['iterations'] == 0)
    assert info0['hessian_passes'] == 0 and np.all(info0['relative_residual'] == 0)
    assert rec.n_solves == before


@pytest.mark.gpu
@pytest.mark.parametrize('kwargs', [dict(field_dtype='single'), dict(keep='host')], ids=['single', 'host'])
def test_storage_variants(kwargs):
    """Against the 'double' / 'device' result within ``2 cond tol`` plus the 1e-6 that ``test_block_products`` allows
    between the storage types."""
    grid, rec, active, act, lams, b, dense = _dense('isotropic')
    maxit = 2 * max(d[3] for d in dense) + 10
    rhs = _to_model(rec, grid, b)
    want = _from_model(rec.gauss_newton_solve(rhs, lams, tol=TOL, maxit=maxit, **REG)[0])
    grid2, other = _survey('isotropic', **kwargs)
    other.forward()
    before = dict(other.n_solves)
    x, info = other.gauss_newton_solve(rhs, lams, tol=TOL, maxit=maxit, **REG)
    x = _from_model(x)
    assert np.all(info['state'] == 1) and other.n_solves == before
    for k, (A, xs, cond, its) in enumerate(dense):
        rel = np.linalg.norm(x[k] - want[k]) / np.linalg.norm(xs)
        record(f"gauss_newton_solve {kwargs}: column {k} |x - x_double| / |x*| = {rel:.2e} (bound {2 * cond * TOL + 1e-6:.2e})")
        assert rel <= 2 * cond * TOL + 1e-6
