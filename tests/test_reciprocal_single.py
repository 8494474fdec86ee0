"""Kept fields stored in single precision: the four ``_sp`` entry points
(``emg3d_dev_sensitivity_dots_sp``, ``emg3d_dev_sensitivity_combine_sp``, ``emg3d_dev_hessian_diagonal_sp``,
``emg3d_dev_data_gram_sp``) through the C ABI against NumPy in fp64 on the widened values, and
``gradient.ReciprocalSensitivity(field_dtype='single')`` against the same class with ``'double'``.

The error model. u = 2^-24, eps = 2^-52. Rounding a kept value to fp32 component-wise gives ``|e~ - e| <= u |e|``, so
a product of two kept values is off by at most ``(2 u + u^2) |e| |x| < 3 u |e| |x|`` and a squared modulus of a sum Z of
such products by at most ``2 |Z| 3 u A + (3 u A)^2 < 7 u A^2``, ``A = sum |e| |x|`` over the same terms. The fp64
summation bounds of the existing kernel tests, ``(terms + c) eps sum |terms|``, add on top. The kernel tests need only
the latter: their reference is computed from the widened values, so storage costs them nothing. Every bound is
computed by NumPy from absolute values: cancellation cannot break it and nothing is tuned.

Inputs, the small survey and the recorder come from ``test_sensitivity``, device helpers from ``test_reciprocal``, the
pair sums and bounds from ``test_hessian_diagonal`` and ``test_data_gram``.
"""
import collections
import functools
import gc

import numpy as np
import pytest

from emg3d_amd import _lib, gradient
from test_data_gram import C_BOUND, FREQS2, SCALE_A, SCALE_B, _panels
from test_hessian_diagonal import ROW_MAPS, _weights, diagonal_and_bound, pair_sums
from test_reciprocal import SIZES, TILES, _dev, _flat, _up
from test_sensitivity import (ADJOINT_CASES, EPS, FREQS, MU_0, OPTS, RECS, SRCS, TOL, _fd_inputs, _maxdiff, _random_data,
                              _stretched, cells_to_edges, record, small_model)

U = 2.0 ** -24
SP_NAMES = ('emg3d_dev_sensitivity_dots_sp', 'emg3d_dev_sensitivity_combine_sp', 'emg3d_dev_hessian_diagonal_sp',
            'emg3d_dev_data_gram_sp')


# ----------------------------------------------------------------------- not gpu tests ---
def test_declared_symbols():
    header = open(_lib.HEADER).read()
    for name in SP_NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name) and name + '(' in header
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name[:-3]]           # the argument list of the sibling


def test_field_dtype_in_the_constructor():
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    assert rec.field_dtype == 'double' and "field_dtype='double'" in repr(rec)
    one = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, field_dtype='single', keep='host')
    assert one.field_dtype == 'single' and "field_dtype='single'" in repr(one) and one.kept_bytes == 0
    assert one.n_solves == {'forward': 0, 'receiver': 0, 'jvec': 0, 'jtvec': 0}
    for bad in ('half', None, np.float32):
        with pytest.raises(ValueError, match="`field_dtype` must be 'double' or 'single'"):
            gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, field_dtype=bad)
    with pytest.raises(TypeError, match="field_dtype"):
        gradient.Sensitivity(model, SRCS, FREQS, RECS, field_dtype='single')


# ------------------------------------------------------------------ kernels on the gpu ---
Stack32 = collections.namedtuple('Stack32', 'wide dev lead stride rows')
ALIGNMENTS = ('odd', 'padded', 'offset')


def _stack32(rng, rows, n, is_complex, align):
    """Random fp32 / complex64 fields in a stack with NaN wherever a kernel must not read (between the rows, before the
    first). ``align``: 'odd' -- an odd stride, so the rows alternate between alignments; 'padded' -- the stride the
    class uses, the next multiple of 16 bytes, from an aligned base; 'offset' -- that stride from a base pointer one
    element behind an aligned address. Returns the widened values (rows, n) and the device buffer."""
    dt = np.complex64 if is_complex else np.float32
    per16 = 16 // np.dtype(dt).itemsize
    stride = (n + 3 + rows) | 1 if align == 'odd' else -(-n // per16) * per16
    lead = 1 if align == 'offset' else 0
    flat = np.full(lead + rows * stride, np.nan, dtype=dt)
    a = flat[lead:].reshape(rows, stride)
    a[:, :n] = rng.standard_normal((rows, n)) + (1j * rng.standard_normal((rows, n)) if is_complex else 0)
    wide = a[:, :n].astype(complex if is_complex else float)
    return Stack32(wide, _up(flat), lead, stride, rows)


def _wide_dtype(is_complex):
    import torch
    return torch.complex128 if is_complex else torch.float64


def _dots_sp(E, X, n, w, scale, is_complex):
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    ws_len = L.emg3d_sensitivity_dots_ws_len(E.rows, X.rows, n)
    ws = torch.full((ws_len,), float('nan'), dtype=torch.float64, device=_dev())
    out = torch.full((E.rows * X.rows,), float('nan'), dtype=_wide_dtype(is_complex), device=_dev())
    _lib.check(L.emg3d_dev_sensitivity_dots_sp(n, int(is_complex), _ptr(E.dev, E.lead), E.stride, E.rows, _ptr(X.dev, X.lead),
                                               X.stride, X.rows, _ptr(w), complex(scale).real, complex(scale).imag, _ptr(out),
                                               _ptr(ws), ws_len, _stream()), 'emg3d_dev_sensitivity_dots_sp')
    return out.cpu().numpy().reshape(E.rows, X.rows)


def _combine_sp(E, X, n, coef, is_complex):
    import torch
    from emg3d_amd._device import _ptr, _stream
    t = torch.full((n,), float('nan'), dtype=_wide_dtype(is_complex), device=_dev())          # every entry must be WRITTEN
    _lib.check(_lib.lib().emg3d_dev_sensitivity_combine_sp(n, int(is_complex), _ptr(E.dev, E.lead), E.stride, E.rows,
                                                           _ptr(X.dev, X.lead), X.stride, X.rows, _ptr(coef), _ptr(t),
                                                           _stream()), 'emg3d_dev_sensitivity_combine_sp')
    return t.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('align', ALIGNMENTS)
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('ns, nr', TILES)
@pytest.mark.parametrize('n', SIZES)
def test_dots_sp_vs_numpy(n, ns, nr, is_complex, align):
    """The bound of ``test_reciprocal.test_dots_vs_numpy``, ``(n + 16) eps |scale| sum_k |w_k| |e_s[k]| |x_r[k]|``, against
    NumPy on the widened values, at the three alignments: 'padded' takes the 16-byte loads, the other two the
    element-wise ones. The largest size is summed a second time: the same bits."""
    rng = np.random.default_rng(n + 10 * ns + nr + is_complex)
    E, X = _stack32(rng, ns, n, is_complex, align), _stack32(rng, nr, n, is_complex, align)
    w = rng.standard_normal(n)
    scale = 0.3 - 1.7j if is_complex else 0.7
    wd = _up(w)
    got = _dots_sp(E, X, n, wd, scale, is_complex)
    want = scale * np.einsum('k,sk,rk->sr', w, E.wide, X.wide)
    bound = (n + 16) * EPS * abs(scale) * np.einsum('k,sk,rk->sr', np.abs(w), np.abs(E.wide), np.abs(X.wide))
    assert got.dtype == (complex if is_complex else float) and not np.any(np.isnan(got))
    worst = float(np.max(np.abs(got - want) / bound))
    record(f"dots_sp n={n} ns={ns} nr={nr} complex={is_complex} {align}: max |diff| / bound = {worst:.2e} "
           f"(bound (n + 16) eps)")
    assert np.all(np.abs(got - want) <= bound)
    if n == SIZES[-1]:
        assert np.array_equal(got, _dots_sp(E, X, n, wd, scale, is_complex))


@pytest.mark.gpu
@pytest.mark.parametrize('align', ALIGNMENTS)
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('ns, nr', TILES + [(2, 11)])
@pytest.mark.parametrize('n', SIZES)
def test_combine_sp_vs_numpy(n, ns, nr, is_complex, align):
    """The bound of ``test_reciprocal.test_combine_vs_numpy``, ``(ns nr + 16) eps sum_{s,r} |e_s[k]| |coef_{s,r}|
    |x_r[k]|`` per entry, at the three alignments; ``t`` starts as NaN and every entry must be written. Twice: the same
    bits."""
    rng = np.random.default_rng(3 * n + 10 * ns + nr + is_complex)
    E, X = _stack32(rng, ns, n, is_complex, align), _stack32(rng, nr, n, is_complex, align)
    coef = rng.standard_normal((ns, nr)) + (1j * rng.standard_normal((ns, nr)) if is_complex else 0)
    cd = _up(coef)
    got = _combine_sp(E, X, n, cd, is_complex)
    want = np.sum(E.wide * (coef @ X.wide), axis=0)
    bound = (ns * nr + 16) * EPS * np.sum(np.abs(E.wide) * (np.abs(coef) @ np.abs(X.wide)), axis=0)
    assert got.dtype == (complex if is_complex else float) and not np.any(np.isnan(got))
    worst = float(np.max(np.abs(got - want) / bound))
    record(f"combine_sp n={n} ns={ns} nr={nr} complex={is_complex} {align}: max |diff| / bound = {worst:.2e} "
           f"(bound (ns nr + 16) eps)")
    assert np.all(np.abs(got - want) <= bound)
    assert np.array_equal(got, _combine_sp(E, X, n, cd, is_complex))


# hessian_diagonal: a workgroup owns 16 x 4 x 4 cells and tiles of 4 x 4 fields -- (19, 6, 7) is ragged along every
# axis, (6, 7) a full and a ragged tile either way. data_gram: patches of 16 x 2 x 2 cells, tiles of 4 x 8 fields.
HD_CASES = [(shape, pair, case) for shape in [(1, 1, 1), (5, 3, 2), (19, 6, 7)] for pair in [(1, 1), (3, 5), (6, 7)]
            for case in ('isotropic', 'triaxial')] + [((19, 6, 7), (3, 5), 'HTI')]


@pytest.mark.gpu
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('shape, pair, case', HD_CASES)
def test_hessian_diagonal_sp_vs_numpy(shape, pair, case, is_complex):
    """The bound of ``test_hessian_diagonal.test_kernel_vs_numpy``, ``(ns nr + 48) eps B`` per cell and row, with its
    set-up: ``h`` starts from random values and has NaN behind each row."""
    from emg3d_amd._device import _ptr, _stream
    ns, nr = pair
    rows = ROW_MAPS[case]
    grid = _stretched(*shape)
    n, ncell, nrows = grid.n_edges, int(np.prod(shape)), max(rows) + 1
    rng = np.random.default_rng(1000 * sum(shape) + 10 * ns + nr + is_complex)
    E, X = _stack32(rng, ns, n, is_complex, 'odd'), _stack32(rng, nr, n, is_complex, 'padded')
    W = rng.uniform(0.1, 2.0, (ns, nr))
    W[rng.random((ns, nr)) < 0.3] = 0.0
    vol = grid.cell_volumes.astype(np.float64)
    Z, S = pair_sums(E.wide, X.wide, shape), pair_sums(np.abs(E.wide), np.abs(X.wide), shape)
    scale = 0.37
    contribution, B = diagonal_and_bound(Z, S, W, rows, scale, vol.reshape(shape, order='F'))
    h0 = np.where(B > 0, rng.uniform(-0.5, 0.5, B.shape) * B, rng.standard_normal(B.shape))
    hs = ncell + 5
    start = np.full((nrows, hs), np.nan)
    start[:, :ncell] = np.stack([r.ravel('F') for r in h0])
    h, Wd, vold = _up(start), _up(W), _up(vol)
    _lib.check(_lib.lib().emg3d_dev_hessian_diagonal_sp(
        *shape, int(is_complex), _ptr(E.dev), E.stride, ns, _ptr(X.dev), X.stride, nr, _ptr(Wd), *rows, scale, _ptr(vold),
        _ptr(h), hs, _stream()), 'emg3d_dev_hessian_diagonal_sp')
    got = h.cpu().numpy().reshape(-1, hs)
    assert np.all(np.isnan(got[:, ncell:])) and not np.any(np.isnan(got[:, :ncell]))
    got3 = np.stack([r.reshape(shape, order='F') for r in got[:, :ncell]])
    bound = (ns * nr + 48) * EPS * B
    diff = np.abs(got3 - (h0 + contribution))
    worst = float(np.max(diff[B > 0] / bound[B > 0])) if np.any(B > 0) else 0.0
    record(f"hessian_diagonal_sp {shape} ns={ns} nr={nr} complex={is_complex} {case}: max |diff| / bound = {worst:.2e} "
           f"(bound (ns nr + 48) eps B)")
    assert np.all(diff <= bound)


GRAM_CASES = [(shape, a, a) for shape in [(1, 1, 1), (5, 2, 2), (19, 5, 3)] for a in [(1, 1), (3, 5), (6, 7)]]
GRAM_CASES += [((19, 5, 3), (3, 5), (2, 9))]                   # two different sides: the non-symmetric path


def _side32(shape, ns, nr, is_complex, seed):
    """``test_data_gram._side`` for narrow stacks: the pair sums of the widened values."""
    n = _stretched(*shape).n_edges
    rng = np.random.default_rng(seed + 1000 * sum(shape) + 10 * ns + nr + is_complex)
    E, X = _stack32(rng, ns, n, is_complex, 'padded'), _stack32(rng, nr, n, is_complex, 'odd')
    Z = [z.reshape(-1, ns * nr) for z in pair_sums(E.wide, X.wide, shape)]
    S = [s.reshape(-1, ns * nr) for s in pair_sums(np.abs(E.wide), np.abs(X.wide), shape)]
    return dict(E=E, X=X, Z=Z, S=S, ns=ns, nr=nr)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['isotropic', 'triaxial'])
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('shape, a, b', GRAM_CASES)
def test_data_gram_sp_vs_numpy(shape, a, b, is_complex, case):
    """The bound of ``test_data_gram.test_kernel_vs_numpy``, ``(nrows n_cells + 40) eps B_ij`` per entry, with its
    set-up (``out`` starts as NaN with ``ld > cols``, ``mw`` has NaN behind every row and exact zeros); with the same
    side twice the block equals its transpose bit for bit."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    rows = ROW_MAPS[case]
    same = a == b
    A = _side32(shape, *a, is_complex, 1)
    B = A if same else _side32(shape, *b, is_complex, 2)
    sa = SCALE_A if is_complex else complex(SCALE_A.real)
    sb = sa if same else SCALE_B if is_complex else complex(SCALE_B.real)
    c = 2 if is_complex else 1
    ncell, nrows = int(np.prod(shape)), max(rows) + 1
    vol = _stretched(*shape).cell_volumes.astype(np.float64).reshape(shape, order='F').ravel()   # C order, as the pair sums
    rng = np.random.default_rng(17 + len(case) + ncell)
    mw = rng.uniform(0.1, 2.0, (nrows, ncell))
    mw[rng.random((nrows, ncell)) < 0.3] = 0.0
    mw[:, 0] = 1.5
    to_f = np.arange(ncell).reshape(shape).ravel(order='F')       # the kernel's cells are x fastest
    mws = ncell + 7
    mw_dev = np.full((nrows, mws), np.nan)
    mw_dev[:, :ncell] = mw[:, to_f]
    JA, SA = _panels(A, rows, sa, is_complex)
    JB, SB = (JA, SA) if same else _panels(B, rows, sb, is_complex)
    wt = (mw * (vol / 4) ** 2).astype(np.longdouble)
    want = np.einsum('pic,pc,pjc->ij', JA, wt, JB)
    bound = ((nrows * ncell + C_BOUND) * EPS * np.einsum('pic,pc,pjc->ij', SA, wt, SB)).astype(float)
    ma, mb = c * a[0] * a[1], c * b[0] * b[1]
    ld = mb + 3
    L = _lib.lib()
    ws_len = L.emg3d_data_gram_ws_len(*shape, int(is_complex), a[0] * a[1], b[0] * b[1])
    ws = torch.full((ws_len,), float('nan'), dtype=torch.float64, device=_dev())
    out, mwd, vold = _up(np.full((ma, ld), np.nan)), _up(mw_dev), _up(vol[to_f])
    _lib.check(L.emg3d_dev_data_gram_sp(
        *shape, int(is_complex), _ptr(A['E'].dev), A['E'].stride, a[0], _ptr(A['X'].dev), A['X'].stride, a[1], sa.real, sa.imag,
        _ptr(B['E'].dev), B['E'].stride, b[0], _ptr(B['X'].dev), B['X'].stride, b[1], sb.real, sb.imag, *rows, _ptr(mwd),
        mws, _ptr(vold), _ptr(out), ld, _ptr(ws), ws_len, _stream()), 'emg3d_dev_data_gram_sp')
    got = out.cpu().numpy()
    assert np.all(np.isnan(got[:, mb:])) and not np.any(np.isnan(got[:, :mb]))
    diff = np.abs(got[:, :mb] - want).astype(float)
    assert np.all(bound > 0)
    record(f"data_gram_sp {shape} A={a} B={b} complex={is_complex} {case}: max |diff| / bound = "
           f"{float(np.max(diff / bound)):.2e} (bound ({nrows} * {ncell} + {C_BOUND}) eps B)")
    assert np.all(diff <= bound)
    if same:
        assert np.array_equal(got[:, :mb], got[:, :mb].T)


@pytest.mark.gpu
def test_sp_entries_refuse_bad_arguments():
    """A null stack, a stride below the row length and a zero count: ``EMG3D_ERR_BADARG`` (-1) with the sibling's
    message, before anything is launched."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    a = torch.zeros(64, dtype=torch.complex64, device=_dev())              # a 2 x 2 x 2 grid: 54 edges, 8 cells
    z = torch.zeros(64, dtype=torch.complex128, device=_dev())
    d = torch.zeros(128, dtype=torch.float64, device=_dev())               # inputs at 0, results from 64 on
    p, q, r, zp, st = _ptr(a), _ptr(d), _ptr(d, 64), _ptr(z), _stream()
    ws_len = L.emg3d_data_gram_ws_len(2, 2, 2, 1, 1, 1)
    gws = torch.zeros(ws_len, dtype=torch.float64, device=_dev())

    def dots(e=p, es=4, ns=1, x=p, xs=4):
        return L.emg3d_dev_sensitivity_dots_sp(4, 1, e, es, ns, x, xs, 1, q, 1., 0., zp, r, 64, st)

    def combine(e=p, es=4, ns=1, x=p, xs=4):
        return L.emg3d_dev_sensitivity_combine_sp(4, 1, e, es, ns, x, xs, 1, zp, zp, st)

    def hessian(e=p, es=54, ns=1, x=p, xs=54):
        return L.emg3d_dev_hessian_diagonal_sp(2, 2, 2, 1, e, es, ns, x, xs, 1, q, 0, 1, 2, 1.0, q, r, 8, st)

    def gram(e=p, es=54, ns=1, x=p, xs=54):
        return L.emg3d_dev_data_gram_sp(2, 2, 2, 1, e, es, ns, x, xs, 1, 1.0, 0.5, p, 54, 1, p, 54, 1, 1.0, 0.5, 0, 1, 2, q, 8, q,
                                        r, 2, _ptr(gws), ws_len, st)
    calls = {'sensitivity_dots': (dots, 3), 'sensitivity_combine': (combine, 3), 'hessian_diagonal': (hessian, 53),
             'data_gram': (gram, 53)}
    for name, (call, short) in calls.items():
        for kw in (dict(e=None), dict(x=None), dict(es=short), dict(xs=short), dict(ns=0)):
            assert call(**kw) == -1, (name, kw)
            with pytest.raises(_lib.Emg3dAmdError, match=f"{name}: "):
                _lib.check(call(**kw), 'emg3d_dev_' + name + '_sp')
    torch.cuda.synchronize()
    assert float(d.abs().sum()) == 0.0 and float(z.abs().sum()) == 0.0 and float(gws.abs().sum()) == 0.0
    for name, (call, _) in calls.items():                                  # (the good call is one)
        _lib.check(call(), 'emg3d_dev_' + name + '_sp')
    torch.cuda.synchronize()


# ------------------------------------------------------------------- the class on the gpu ---
CASES = {name: ADJOINT_CASES[name] for name in ('isotropic-resistivity', 'triaxial-LgResistivity')}
CASES['laplace'] = dict(case='isotropic', mapping='Resistivity', freqs={'f': -1.0})
CASES['two-frequencies'] = dict(case='isotropic', mapping='Conductivity', freqs=FREQS2)


def _bits(t):
    """A stack's values as unsigned integers: equality of these is equality bit for bit."""
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)           # complex64 / float32


@functools.lru_cache(maxsize=None)
def _instances(name):
    """One case, once: its grid and model and three instances after ``forward()`` -- 'double', 'single', and 'wide', a
    'double' one whose stacks are overwritten by the widened values of 'single': it computes from the very same
    numbers, in fp64 storage."""
    spec = CASES[name]
    grid, model = small_model(spec['case'], spec['mapping'])
    freqs = spec.get('freqs', FREQS)
    kw = dict(solver_opts=OPTS, tol_gradient=TOL)
    out = {k: gradient.ReciprocalSensitivity(model, SRCS, freqs, RECS, field_dtype=d, **kw).forward()
           for k, d in (('double', 'double'), ('single', 'single'), ('wide', 'double'))}
    for fname, stacks in out['wide']._stacks.items():
        for wide, narrow in zip(stacks, out['single']._stacks[fname]):
            wide.copy_(narrow.to(wide.dtype))
    return dict(out, grid=grid, model=model, freqs=freqs, spec=spec)


def _smu0(freq):
    return 2j * np.pi * freq * MU_0 if freq > 0 else -freq * MU_0


def _chain(model, spec, shape):
    return np.stack([gradient._DCHAIN[spec['mapping']](np.ones(shape), np.asarray(getattr(model, prop), dtype=float))
                     for prop in gradient._PROPS[spec['case']]])


def _jvec_magnitudes(d, rec, v):
    """``|s mu0| sum_k w_k(|v| |chain|) |e_s[k]| |x_r[k]|`` per pair, from the stacks of ``rec``: dict pair -> (nrec,)."""
    grid, model = d['grid'], d['model']
    shape = tuple(grid.shape_cells)
    vol = grid.cell_volumes.reshape(shape, order='F')
    w = _flat(cells_to_edges(vol[None] * np.abs(gradient.expand_vector(model, np.abs(v)))))     # (with the chain)
    out = {}
    for fname, mine, *_ in rec._per_frequency():
        E, X = (np.abs(t.cpu().numpy().astype(complex)) for t in rec._stacks[fname])
        mag = abs(_smu0(d['freqs'][fname])) * np.einsum('k,sk,rk->sr', w, E, X)
        out.update({rec.pairs[i]: mag[row] for row, i in enumerate(mine)})
    return out


def _hessian_B(d, rec, w):
    """The B of ``test_hessian_diagonal`` times chain^2, shaped like ``hessian_diagonal``'s result, from the stacks of
    ``rec`` (one frequency 'f'): ``scale (V / 4)^2 sum_{s,r} w A^2 chain^2``, A the pair sums of magnitudes."""
    grid, model, spec = d['grid'], d['model'], d['spec']
    shape = tuple(grid.shape_cells)
    W = np.stack([np.nan_to_num(w.get(p, np.zeros(len(RECS)))) for p in rec.pairs])
    E, X = (np.abs(t.cpu().numpy().astype(complex)) for t in rec._stacks['f'])
    S = pair_sums(E, X, shape)
    _, B = diagonal_and_bound(S, S, W, ROW_MAPS[spec['case']], abs(_smu0(d['freqs']['f'])) ** 2,
                              grid.cell_volumes.reshape(shape, order='F'))
    return B * _chain(model, spec, shape) ** 2


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['isotropic-resistivity', 'laplace'])
def test_narrowing_is_a_cast_and_nothing_else(name):
    """Every stack of 'single' is the stack of 'double' cast to complex64 (Laplace domain: float32), bit for bit;
    ``kept_bytes`` is what the stacks hold: half of the double figure plus the padding of the rows to 16 bytes (at most
    8 bytes per complex64 row, 12 per float32 row); responses, solve counts and the keys of ``info`` are those of
    'double'; the results of ``jvec`` have today's type."""
    import torch
    d = _instances(name)
    dbl, sgl, n = d['double'], d['single'], d['grid'].n_edges
    narrow = torch.float32 if name == 'laplace' else torch.complex64
    size = 4 if name == 'laplace' else 8
    held, rows = 0, 0
    for fname, stacks in sgl._stacks.items():
        for t, ref in zip(stacks, dbl._stacks[fname]):
            assert t.dtype == narrow and t.shape == ref.shape and t.data_ptr() % 16 == 0 and t.stride(0) * size % 16 == 0
            assert np.array_equal(_bits(t), _bits(ref.to(narrow)))
            held += len(t) * t.stride(0) * size
            rows += len(t)
    assert rows == 5 and sgl.kept_bytes == held == 5 * (-(-n * size // 16) * 16)
    assert dbl.kept_bytes == 5 * n * 2 * size
    assert sgl.kept_bytes <= dbl.kept_bytes // 2 + rows * (16 - size)
    assert f"{sgl.kept_bytes:,} B" in repr(sgl) and "field_dtype='single'" in repr(sgl)
    assert all(np.array_equal(sgl.synthetic[p], dbl.synthetic[p]) for p in dbl.pairs) and list(sgl.synthetic) == dbl.pairs
    assert sgl.n_solves == dbl.n_solves == {'forward': 2, 'receiver': 3, 'jvec': 0, 'jtvec': 0}
    assert set(sgl.info) == set(dbl.info)
    v = np.random.default_rng(11).standard_normal(d['grid'].shape_cells)
    js, jd = sgl.jvec(v), dbl.jvec(v)
    assert all(js[p].dtype == jd[p].dtype and js[p].shape == jd[p].shape for p in dbl.pairs)
    assert all(np.iscomplexobj(js[p]) == (name != 'laplace') for p in dbl.pairs)
    record(f"kept_bytes, {name}: double {dbl.kept_bytes:,} B, single {sgl.kept_bytes:,} B; jvec single vs double "
           f"{_maxdiff(js, jd):.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['isotropic-resistivity', 'triaxial-LgResistivity'])
def test_wiring_jvec_and_hessian_diagonal(name):
    """'single' against 'wide' -- the same numbers in fp64 storage, so only the order of summation may differ:
    ``jvec`` within ``(n_edges + 16) eps |scale| sum |w| |e| |x|`` per entry, ``hessian_diagonal`` within the kernel
    test's ``(ns nr + 48) eps B chain^2`` per cell."""
    d = _instances(name)
    sgl, wide, grid = d['single'], d['wide'], d['grid']
    rng = np.random.default_rng(19)
    v = rng.standard_normal((gradient._NCOMP[d['spec']['case']],) + tuple(grid.shape_cells))
    js, jw = sgl.jvec(v), wide.jvec(v)
    mag = _jvec_magnitudes(d, wide, v)
    worst = 0.0
    for p in sgl.pairs:
        bound = (grid.n_edges + 16) * EPS * mag[p]
        worst = max(worst, float(np.max(np.abs(js[p] - jw[p]) / bound)))
        assert np.all(np.abs(js[p] - jw[p]) <= bound)
    w = _weights(np.random.default_rng(71))
    Hs, Hw = sgl.hessian_diagonal(w), wide.hessian_diagonal(w)
    bound = ((len(SRCS) * len(RECS) + 48) * EPS * _hessian_B(d, wide, w)).reshape(Hw.shape)
    record(f"single vs the same values in fp64 storage, {name}: jvec max |diff| / bound = {worst:.2e} (bound (n_edges + "
           f"16) eps); hessian_diagonal max |diff| / bound = {float(np.max(np.abs(Hs - Hw) / bound)):.2e} (bound (ns nr + "
           f"48) eps B), bit-identical: {np.array_equal(Hs, Hw)}")
    assert Hs.shape == Hw.shape and Hs.dtype == np.float64 and np.all(bound > 0)
    assert np.all(np.abs(Hs - Hw) <= bound)
    assert sgl.n_solves == {'forward': 2, 'receiver': 3, 'jvec': 0, 'jtvec': 0}


@pytest.mark.gpu
def test_wiring_jtvec_and_data_gram_are_pinned_to_jvec():
    """On the 'single' instance itself, two frequencies, mapping 'Conductivity'. (a) Adjointness to rounding, as
    ``test_reciprocal.test_products_are_adjoint_to_rounding``: ``|sum v jtvec(y) - Re sum conj(y) jvec(v)| <= (n_edges
    + 64) eps S`` -- both products read the same narrow values. (b) The identities of ``data_gram``'s docstring with the
    bound matrix of ``test_data_gram`` (``(nrows n_cells + 40) eps B_ij``, twice for matrix against the ``jtvec``
    route, three times for matrix times data against ``jvec``):
    ``|ys @ G @ zs - sum m jtvec(y) jtvec(z)| <= |ys| @ (2 bound) @ |zs|`` and
    ``|G @ ys - stack_data(jvec(m jtvec(y)))| <= 3 bound @ |ys|``."""
    d = _instances('two-frequencies')
    rec, grid, model = d['single'], d['grid'], d['model']
    shape = tuple(grid.shape_cells)
    nrec = len(RECS)
    rng = np.random.default_rng(53)
    v = rng.standard_normal((1,) + shape)
    y = _random_data(rng, rec.pairs, nrec)
    y[rec.pairs[1]][2] = np.nan
    jv, jt = rec.jvec(v), rec.jtvec(y)
    lhs = float(np.sum(v.reshape(jt.shape) * jt))
    rhs = float(sum(np.nansum(np.conj(y[p]) * jv[p]).real for p in rec.pairs))
    mag = _jvec_magnitudes(d, rec, v)
    S = float(sum(np.sum(np.abs(np.nan_to_num(y[p])) * mag[p]) for p in rec.pairs))
    bound = (grid.n_edges + 64) * EPS * S
    record(f"single, adjoint to rounding: sum(v jtvec(y)) {lhs:.15e}  Re sum conj(y) jvec(v) {rhs:.15e}  |diff| "
           f"{abs(lhs - rhs):.2e} = {abs(lhs - rhs) / bound:.2e} x bound ((n_edges + 64) eps S)")
    assert abs(lhs - rhs) <= bound
    # (b)
    m = rng.uniform(0.1, 2.0, shape)
    m[rng.random(shape) < 0.2] = 0.0
    G = rec.data_gram(m)
    N = len(rec.pairs) * nrec
    Smag = np.zeros((1, N, grid.n_cells))
    for fname, mine, *_ in rec._per_frequency():
        E, X = (np.abs(t.cpu().numpy().astype(complex)) for t in rec._stacks[fname])
        Sd = [s.reshape(-1, len(mine), nrec) for s in pair_sums(E, X, shape)]
        sp = abs(_smu0(d['freqs'][fname])) * sum(Sd)                       # isotropic: one row for the three directions
        for row, k in enumerate(mine):
            Smag[0, k * nrec:(k + 1) * nrec] = sp[:, row, :].T
    chain = _chain(model, d['spec'], shape)
    wt = (m * chain ** 2 * (grid.cell_volumes.reshape(shape, order='F') / 4) ** 2).reshape(1, -1)
    Smag = np.concatenate([Smag] * 2, axis=1)
    gbound = (grid.n_cells + C_BOUND) * EPS * np.einsum('pic,pc,pjc->ij', Smag, wt, Smag)
    z = _random_data(rng, rec.pairs, nrec)
    del z[rec.pairs[2]]
    ys, zs = rec.stack_data(y), rec.stack_data(z)
    jz = rec.jtvec(z)
    left, right = float(ys @ G @ zs), float(np.sum(m * jt * jz))
    tol = float(np.abs(ys) @ (2 * gbound) @ np.abs(zs))
    record(f"single, ys @ G @ zs {left:.15e} vs sum m jtvec(y) jtvec(z) {right:.15e}: |diff| / tolerance = "
           f"{abs(left - right) / tol:.2e}")
    assert G.shape == (2 * N, 2 * N) and np.array_equal(G, G.T)
    assert abs(left - right) <= tol
    gy, jj = G @ ys, rec.stack_data(rec.jvec(m * jt))
    tol = 3 * gbound @ np.abs(ys)
    record(f"single, G @ ys vs stack_data(jvec(m jtvec(y))): max |diff| / (3 sum bound |y|) = "
           f"{float(np.max(np.abs(gy - jj) / tol)):.2e}")
    assert np.all(np.abs(gy - jj) <= tol)
    assert rec.n_solves == {'forward': 4, 'receiver': 6, 'jvec': 0, 'jtvec': 0}


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['isotropic-resistivity', 'triaxial-LgResistivity'])
def test_single_against_true_double(name):
    """Per entry ``|jvec_single - jvec_double| <= (3 u + (n_edges + 16) eps) |scale| sum |w| |e| |x|`` and per cell
    ``|H_single - H_double| <= (7 u + (ns nr + 48) eps) scale (V / 4)^2 sum w A^2 chain^2`` (module docstring; the
    magnitudes from the fields of 'double'). The differences of ``jtvec``, ``data_gram`` and ``misfit_and_gradient``
    are recorded: ``test_wiring_jtvec_and_data_gram_are_pinned_to_jvec`` ties them to ``jvec``."""
    d = _instances(name)
    sgl, dbl, grid = d['single'], d['double'], d['grid']
    ncomp = gradient._NCOMP[d['spec']['case']]
    rng = np.random.default_rng(29)
    v = rng.standard_normal((ncomp,) + tuple(grid.shape_cells))
    js, jd = sgl.jvec(v), dbl.jvec(v)
    mag = _jvec_magnitudes(d, dbl, v)
    worst_j = 0.0
    for p in dbl.pairs:
        bound = (3 * U + (grid.n_edges + 16) * EPS) * mag[p]
        worst_j = max(worst_j, float(np.max(np.abs(js[p] - jd[p]) / bound)))
        assert np.all(np.abs(js[p] - jd[p]) <= bound)
    w = _weights(np.random.default_rng(71))
    Hs, Hd = sgl.hessian_diagonal(w), dbl.hessian_diagonal(w)
    bound = ((7 * U + (len(SRCS) * len(RECS) + 48) * EPS) * _hessian_B(d, dbl, w)).reshape(Hd.shape)
    worst_h = float(np.max(np.abs(Hs - Hd) / bound))
    y = _random_data(rng, dbl.pairs, len(RECS))
    dt = _maxdiff(sgl.jtvec(y), dbl.jtvec(y))
    dg = _maxdiff(sgl.data_gram(), dbl.data_gram())
    record(f"single vs double, {name}: jvec max |diff| / bound = {worst_j:.2e} (bound 3 u + (n_edges + 16) eps), max-norm "
           f"relative {_maxdiff(js, jd):.2e}; hessian_diagonal max |diff| / bound = {worst_h:.2e} (bound 7 u + (ns nr + 48) "
           f"eps), max-norm relative {_maxdiff(Hs, Hd):.2e}; jtvec {dt:.2e}; data_gram {dg:.2e} (max-norm relative)")
    assert np.all(bound > 0) and np.all(np.abs(Hs - Hd) <= bound)
    if name == 'isotropic-resistivity':
        _, _, obs, wts = _fd_inputs()
        (m0, g0), (m1, g1) = dbl.misfit_and_gradient(obs, wts), sgl.misfit_and_gradient(obs, wts)
        record(f"single vs double, misfit_and_gradient: misfit {'the same bits' if m0 == m1 else abs(m1 - m0) / m0}, "
               f"gradient {_maxdiff(g1, g0):.2e} (max-norm relative)")
        assert m0 == m1                                                    # from the responses, which are not narrowed


@pytest.mark.gpu
def test_host_kept_single_fields_and_release():
    """``keep='host'`` with 'single': pinned complex64 stacks, the five products bit for bit those of ``keep='device'``
    (two frequencies: the second staging pair of ``data_gram`` is part of it), and ``release()`` returns every byte."""
    import torch
    d = _instances('two-frequencies')
    dev, grid, model = d['single'], d['grid'], d['model']
    rng = np.random.default_rng(61)
    v = rng.standard_normal(grid.shape_cells)
    y = _random_data(rng, dev.pairs, len(RECS))
    w = {p: rng.uniform(0.1, 2.0, len(RECS)) for p in dev.pairs}

    def products(rec):
        return [rec.jvec(v), rec.jtvec(y), rec.hessian_diagonal(w), rec.hessian_vec(v, w), rec.data_gram()]
    want = products(dev)
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    host = gradient.ReciprocalSensitivity(model, SRCS, FREQS2, RECS, solver_opts=OPTS, tol_gradient=TOL, keep='host',
                                          field_dtype='single')
    got = products(host)
    assert all(t.dtype == torch.complex64 and t.device.type == 'cpu' and t.is_pinned()
               for st in host._stacks.values() for t in st)
    assert all(t.dtype == torch.complex64 and t.device.type == 'cuda' for t in host._stage) and len(host._stage) == 2
    assert host.kept_bytes == dev.kept_bytes and host.n_solves == dev.n_solves
    assert sum(t.numel() * t.element_size() for t in host._stage) == dev.kept_bytes // 2       # one frequency at a time
    for name, a, b in zip(('jvec', 'jtvec', 'hessian_diagonal', 'hessian_vec', 'data_gram'), got, want):
        same = all(np.array_equal(a[p], b[p]) for p in b) if isinstance(b, dict) else np.array_equal(a, b)
        record(f"single, keep='host' vs keep='device', {name}: bit-identical: {same}")
        assert same
    held = torch.cuda.memory_allocated()
    host.release()
    del got
    gc.collect()
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    record(f"release(), single on the host: allocated {held:,} B -> {after:,} B; before construction {before:,} B")
    assert host.kept_bytes == 0 and after == before
