"""Block sensitivity products: the two kernels of ``csrc/block.h`` (``emg3d_dev_sensitivity_dots_block``,
``emg3d_dev_sensitivity_combine_block`` and their ``_sp`` siblings) through the C ABI against NumPy written out in this
file and, column by column, against the single-vector entry points; and ``jvec_block`` / ``jtvec_block`` /
``hessian_vec_block`` of ``gradient.ReciprocalSensitivity`` against K calls of ``jvec`` / ``jtvec`` / ``hessian_vec``.

The bounds. Kernels: the worst case of ANY order of summation, as ``test_reciprocal`` has it -- ``(n + 16) eps |scale|
sum_k |w_k| |e_s[k]| |x_r[k]|`` for a dot, ``(ns nr + 16) eps sum_{s,r} |e_s[k]| |coef_{s,r}| |x_r[k]|`` for a combined
edge --, computed by NumPy from absolute values; ``combine_block`` must in addition equal ``combine`` bit for bit.
Methods: bit equality where the same kernels run in the same order on the same bits (``jtvec_block``, the device route),
``1e-10`` of the max-norm where sums are reordered (DESIGN.md 4.12 observes 6e-16 on these sizes), ``1e-12`` for
adjointness, ``1e-6`` between the two storage types (DESIGN.md 4.15 observes 5e-8).

Inputs, the small survey and the recorder come from ``test_sensitivity``, device helpers from ``test_reciprocal``.
"""
import functools

import numpy as np
import pytest

from emg3d_amd import _lib, gradient
from test_reciprocal import _comp_grid, _dev, _up
from test_sensitivity import ADJOINT_CASES, EPS, FREQS, OPTS, RECS, SRCS, TOL, _maxdiff, _random_data, record, small_model

SYMBOLS = ('emg3d_sensitivity_dots_block_ws_len', 'emg3d_dev_sensitivity_dots_block', 'emg3d_dev_sensitivity_combine_block',
           'emg3d_dev_sensitivity_dots_block_sp', 'emg3d_dev_sensitivity_combine_block_sp')
NONE = {'forward': 0, 'receiver': 0, 'jvec': 0, 'jtvec': 0}


# ----------------------------------------------------------------------- not gpu tests ---
def test_declared_symbols_and_public_methods():
    header = open(_lib.HEADER).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name) and name + '(' in header
    for name in SYMBOLS[1:3]:
        assert _lib.SIGNATURES[name + '_sp'] == _lib.SIGNATURES[name]          # the argument list of the sibling
    for name in ('jvec_block', 'jtvec_block', 'hessian_vec_block', 'to_device', 'from_device'):
        assert callable(getattr(gradient.ReciprocalSensitivity, name))


def _message(call, kind=ValueError):
    with pytest.raises(kind) as err:
        call()
    return str(err.value)


@pytest.mark.parametrize('case, n', [('isotropic', 1), ('HTI', 2), ('triaxial', 3)])
def test_blocks_are_validated_before_any_gpu_work(case, n):
    """K = 0, a wrong trailing shape, complex vectors, a tensor that is no device block, data that are no sequence of
    dictionaries with one value per receiver, and a bad ``columns_per_pass``: ``ValueError`` in the words of
    ``_check_vector`` / ``_check_data``, raised without a device (before ``require_gpu``)."""
    import torch
    grid, model = small_model(case)
    shape = tuple(grid.shape_cells)
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    good = (n,) + shape
    bad_blocks = [np.zeros((0,) + good), np.zeros((2, n + 1) + shape), np.zeros((2,) + shape[:2]), np.zeros(good[1:]),
                  np.zeros((2,) + good, dtype=complex), np.float64(1.0)]
    if n > 1:
        bad_blocks.append(np.zeros((2,) + shape))
    ncell = grid.n_cells
    bad_tensors = [torch.zeros((2, n, ncell), dtype=torch.float64),                          # not on the device
                   torch.zeros((2, n, ncell), dtype=torch.float32), torch.zeros((2, n, ncell + 1), dtype=torch.float64),
                   torch.zeros((0, n, ncell), dtype=torch.float64), torch.zeros((2, n * ncell), dtype=torch.float64),
                   torch.zeros((2, ncell, n), dtype=torch.float64).permute(0, 2, 1)]
    for method in (rec.jvec_block, rec.hessian_vec_block, rec.to_device):
        for bad in bad_blocks:
            text = _message(lambda: method(bad))
            assert "`vectors` must be real with shape" in text and f"case '{case}'" in text and "Provided:" in text
    for method in (rec.jvec_block, rec.hessian_vec_block, rec.from_device):
        for bad in bad_tensors:
            text = _message(lambda: method(bad))
            assert "a device block must be a contiguous float64 tensor" in text and f"(K, {n}, {ncell})" in text
    nrec = len(RECS)
    y = {('a', 'f'): np.zeros(nrec + 1, dtype=complex)}
    assert _message(lambda: rec.jtvec_block([{}, y])) == _message(lambda: rec.jtvec(y))
    assert "one value per receiver" in _message(lambda: rec.jtvec_block([y]))
    for bad in ([], (), {}, y, None):
        assert "sequence of K >= 1 data dictionaries" in _message(lambda: rec.jtvec_block(bad))
    w = {('a', 'f'): -np.ones(nrec)}
    assert _message(lambda: rec.hessian_vec_block(np.zeros((2,) + good), w)) == _message(lambda: rec.hessian_diagonal(w))
    for bad in (0, -1, 2.0, None, True):
        for call in (lambda: rec.jvec_block(np.zeros((2,) + good), columns_per_pass=bad),
                     lambda: rec.jtvec_block([{}], columns_per_pass=bad),
                     lambda: rec.hessian_vec_block(np.zeros((2,) + good), columns_per_pass=bad)):
            assert "`columns_per_pass` must be an integer >= 1" in _message(call)
    assert rec.n_solves == NONE and rec.kept_bytes == 0


def test_no_cpu_fallback_without_gpu():
    if _lib.lib().emg3d_device_count() > 0:
        pytest.skip("GPU present")
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    v = np.ones((2,) + tuple(grid.shape_cells))
    for call in (lambda: rec.jvec_block(v), lambda: rec.jtvec_block([{('a', 'f'): np.ones(3, dtype=complex)}]),
                 lambda: rec.hessian_vec_block(v), lambda: rec.to_device(v)):
        assert "no HIP device" in _message(call, _lib.Emg3dAmdError)


# ------------------------------------------------------------------ kernels on the gpu ---
SIZES = [1, 257, 1024, 8197, 3 * 8192 + 1]   # one lane; past one workgroup of combine; a multiple of every pack (2, 4):
                                             # no ragged tail; ragged chunks of dots (8192) and of dots_block (4096):
                                             # two and three; several
TILES = [(1, 1), (3, 5), (5, 9)]       # ragged against the 2 x 4 tile of dots_block (and 4 x 4 of dots), past CMB_XR = 8
VECTORS = [1, 3, 9, 19]                # 9: > 2 x 4, the vector tile of dots_block; 19: > 2 x 8, that of combine_block
# 'sp-aligned': every row of the stacks, of w and of t on a 16-byte boundary -- the 16-byte loads (and packed stores of t)
# run, for real and complex fields; 'sp-odd': odd strides everywhere -- element-wise; 'sp-mixed': the stacks aligned, the
# rows of w and t on odd strides -- the launcher must fall back on the strength of w (dots_block) or t (combine_block, real
# fields; rows of complex128 are on 16 bytes whatever the stride) alone
STORAGE = ['fp64', 'sp-aligned', 'sp-odd', 'sp-mixed']


def _rows(rng, rows, n, dtype, aligned):
    """(rows, stride) of ``dtype`` with stride > n: random values, NaN behind every row, which must never be read.
    ``aligned``: every row starts on a 16-byte boundary; otherwise the stride is odd."""
    size = np.dtype(dtype).itemsize
    per16 = max(16 // size, 1)
    stride = -(-(n + 1) // per16) * per16 if aligned else (n + 3 + rows) | 1
    a = np.full((rows, stride), np.nan, dtype=dtype)
    a[:, :n] = rng.standard_normal((rows, n)) + (1j * rng.standard_normal((rows, n)) if np.dtype(dtype).kind == 'c' else 0)
    return a, stride


def _inputs(seed, n, ns, nr, nv, is_complex, storage):
    """Stacks E, X (as stored), their widened values, and the weight rows W, all with strides > n and NaN padding."""
    rng = np.random.default_rng(seed)
    wide = complex if is_complex else float
    stored = wide if storage == 'fp64' else (np.complex64 if is_complex else np.float32)
    aligned = storage != 'sp-odd'
    rows_aligned = aligned and storage != 'sp-mixed'                          # (the rows of w and of t)
    (E, es), (X, xs) = _rows(rng, ns, n, stored, aligned), _rows(rng, nr, n, stored, aligned)
    W, wst = _rows(rng, nv, n, float, rows_aligned)
    t_stride = n + 2 + n % 2 if rows_aligned else (n + 4) | 1                 # even (float64 rows on 16 bytes) or odd, > n
    return dict(E=E, es=es, X=X, xs=xs, W=W, wst=wst, Ew=E[:, :n].astype(wide), Xw=X[:, :n].astype(wide), wide=wide,
                sp='' if storage == 'fp64' else '_sp', t_stride=t_stride)


def _tdtype(is_complex):
    import torch
    return torch.complex128 if is_complex else torch.float64


def _dots_block(d, Ed, Xd, Wd, n, nv, scale, is_complex, short=0, check=True):
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    ns, nr = len(d['E']), len(d['X'])
    ws_len = L.emg3d_sensitivity_dots_block_ws_len(ns, nr, nv, n)
    ws = torch.full((ws_len,), float('nan'), dtype=torch.float64, device=_dev())
    out = torch.full((nv * ns * nr,), float('nan'), dtype=_tdtype(is_complex), device=_dev())
    name = 'emg3d_dev_sensitivity_dots_block' + d['sp']
    status = getattr(L, name)(n, int(is_complex), _ptr(Ed), d['es'], ns, _ptr(Xd), d['xs'], nr, _ptr(Wd), d['wst'], nv,
                              complex(scale).real, complex(scale).imag, _ptr(out), _ptr(ws), ws_len - short, _stream())
    if not check:
        return status
    _lib.check(status, name)
    return out.cpu().numpy().reshape(nv, ns, nr)


def _dots_single(d, Ed, Xd, Wd, n, v, scale, is_complex):
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    ns, nr = len(d['E']), len(d['X'])
    ws_len = L.emg3d_sensitivity_dots_ws_len(ns, nr, n)
    ws = torch.full((ws_len,), float('nan'), dtype=torch.float64, device=_dev())
    out = torch.full((ns * nr,), float('nan'), dtype=_tdtype(is_complex), device=_dev())
    name = 'emg3d_dev_sensitivity_dots' + d['sp']
    _lib.check(getattr(L, name)(n, int(is_complex), _ptr(Ed), d['es'], ns, _ptr(Xd), d['xs'], nr, _ptr(Wd, v * d['wst']),
                                complex(scale).real, complex(scale).imag, _ptr(out), _ptr(ws), ws_len, _stream()), name)
    return out.cpu().numpy().reshape(ns, nr)


@pytest.mark.gpu
@pytest.mark.parametrize('storage', STORAGE)
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('nv', VECTORS)
@pytest.mark.parametrize('ns, nr', TILES)
@pytest.mark.parametrize('n', SIZES)
def test_dots_block_vs_numpy_and_dots(n, ns, nr, nv, is_complex, storage):
    """``|got - want| <= (n + 16) eps |scale| sum_k |w_v[k]| |e_s[k]| |x_r[k]|`` per entry, against NumPy on the widened
    values and, column by column, against ``emg3d_dev_sensitivity_dots`` with row v of w; a second call gives the same
    bits; no NaN (padding) reaches an output; a workspace one element short is refused."""
    d = _inputs(n + 10 * ns + nr + 100 * nv + is_complex, n, ns, nr, nv, is_complex, storage)
    scale = 0.3 - 1.7j if is_complex else 0.7
    Ed, Xd, Wd = _up(d['E']), _up(d['X']), _up(d['W'])
    got = _dots_block(d, Ed, Xd, Wd, n, nv, scale, is_complex)
    W = d['W'][:, :n]
    P = (d['Ew'][:, None, :] * d['Xw'][None, :, :]).reshape(ns * nr, n)
    want = scale * (W @ P.T).reshape(nv, ns, nr)
    bound = (n + 16) * EPS * abs(scale) * (np.abs(W) @ np.abs(P).T).reshape(nv, ns, nr)
    assert got.dtype == d['wide'] and not np.any(np.isnan(got))
    single = np.stack([_dots_single(d, Ed, Xd, Wd, n, v, scale, is_complex) for v in range(nv)])
    worst = [float(np.max(np.abs(got - ref) / bound)) for ref in (want, single)]
    record(f"dots_block n={n} ns={ns} nr={nr} nv={nv} complex={is_complex} {storage}: max |diff| / bound = {worst[0]:.2e} vs "
           f"NumPy, {worst[1]:.2e} vs dots per column (bound (n + 16) eps)")
    assert np.all(np.abs(got - want) <= bound) and np.all(np.abs(got - single) <= bound)
    assert np.array_equal(got, _dots_block(d, Ed, Xd, Wd, n, nv, scale, is_complex))
    assert _dots_block(d, Ed, Xd, Wd, n, nv, scale, is_complex, short=1, check=False) == -1


def _combine_block(d, Ed, Xd, cd, n, nv, is_complex):
    """t as (nv, t_stride) with NaN everywhere before the call: every entry of a row must be WRITTEN, no other."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    ts = d['t_stride']
    t = torch.full((nv, ts), float('nan'), dtype=_tdtype(is_complex), device=_dev())
    before = t.cpu().numpy().copy()
    name = 'emg3d_dev_sensitivity_combine_block' + d['sp']
    _lib.check(getattr(_lib.lib(), name)(n, int(is_complex), _ptr(Ed), d['es'], len(d['E']), _ptr(Xd), d['xs'], len(d['X']),
                                         _ptr(cd), nv, _ptr(t), ts, _stream()), name)
    after = t.cpu().numpy()
    assert after[:, n:].tobytes() == before[:, n:].tobytes()                  # no byte of the padding has changed
    return t[:, :n]


def _combine_single(d, Ed, Xd, cd, n, v, is_complex):
    import torch
    from emg3d_amd._device import _ptr, _stream
    ns, nr = len(d['E']), len(d['X'])
    t = torch.full((n,), float('nan'), dtype=_tdtype(is_complex), device=_dev())
    name = 'emg3d_dev_sensitivity_combine' + d['sp']
    _lib.check(getattr(_lib.lib(), name)(n, int(is_complex), _ptr(Ed), d['es'], ns, _ptr(Xd), d['xs'], nr,
                                         _ptr(cd, v * ns * nr), _ptr(t), _stream()), name)
    return t


@pytest.mark.gpu
@pytest.mark.parametrize('storage', STORAGE)
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('nv', VECTORS)
@pytest.mark.parametrize('ns, nr', TILES)
@pytest.mark.parametrize('n', SIZES)
def test_combine_block_vs_numpy_and_combine(n, ns, nr, nv, is_complex, storage):
    """Row v is ``emg3d_dev_sensitivity_combine`` with ``coef[v]`` bit for bit (``torch.equal``), and within ``(ns nr +
    16) eps sum_{s,r} |e_s[k]| |coef_{v,s,r}| |x_r[k]|`` of NumPy on the widened values; every entry of a row is written
    (t starts as NaN) and no byte between the rows."""
    import torch
    d = _inputs(3 * n + 10 * ns + nr + 100 * nv + is_complex, n, ns, nr, nv, is_complex, storage)
    rng = np.random.default_rng(n + ns + nr + nv)
    coef = rng.standard_normal((nv, ns, nr)) + (1j * rng.standard_normal((nv, ns, nr)) if is_complex else 0)
    Ed, Xd, cd = _up(d['E']), _up(d['X']), _up(coef)
    t = _combine_block(d, Ed, Xd, cd, n, nv, is_complex)
    got = t.cpu().numpy()
    want = np.sum(d['Ew'][None] * (coef.reshape(nv * ns, nr) @ d['Xw']).reshape(nv, ns, n), axis=1)
    bound = (ns * nr + 16) * EPS * np.sum(np.abs(d['Ew'])[None] * (np.abs(coef).reshape(nv * ns, nr) @
                                                                   np.abs(d['Xw'])).reshape(nv, ns, n), axis=1)
    assert got.dtype == d['wide'] and not np.any(np.isnan(got))
    worst = float(np.max(np.abs(got - want) / bound))
    same = all(torch.equal(t[v], _combine_single(d, Ed, Xd, cd, n, v, is_complex)) for v in range(nv))
    record(f"combine_block n={n} ns={ns} nr={nr} nv={nv} complex={is_complex} {storage}: max |diff| / bound = {worst:.2e} "
           f"(bound (ns nr + 16) eps); rows bit-identical to combine: {same}")
    assert np.all(np.abs(got - want) <= bound)
    assert same


@pytest.mark.gpu
def test_block_entries_refuse_bad_arguments():
    """Null pointers, ``nv < 1``, a stride below ``n`` and a short workspace: ``EMG3D_ERR_BADARG`` (-1) with the entry's
    name, before anything is launched (no output moves); the good call is one."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    z = torch.zeros(64, dtype=torch.complex128, device=_dev())
    a = torch.zeros(64, dtype=torch.complex64, device=_dev())
    d = torch.zeros(128, dtype=torch.float64, device=_dev())                  # w at 0, the workspace from 64 on
    o = torch.zeros(64, dtype=torch.complex128, device=_dev())
    st = _stream()
    need = L.emg3d_sensitivity_dots_block_ws_len(1, 1, 2, 4)
    assert need == 2 * 2 and L.emg3d_sensitivity_dots_block_ws_len(3, 5, 9, 3 * 8192 + 1) == 2 * 9 * 15 * 7
    assert all(L.emg3d_sensitivity_dots_block_ws_len(*bad) == 0 for bad in ((0, 1, 1, 4), (1, 0, 1, 4), (1, 1, 0, 4),
                                                                             (1, 1, 1, 0)))
    for sp, p in (('', _ptr(z)), ('_sp', _ptr(a))):
        def dots(e=p, es=4, x=p, xs=4, w=_ptr(d), wst=4, nv=2, out=_ptr(o), ws=_ptr(d, 64), ws_len=need, ns=1):
            return getattr(L, 'emg3d_dev_sensitivity_dots_block' + sp)(4, 1, e, es, ns, x, xs, 1, w, wst, nv, 1., 0., out, ws,
                                                                       ws_len, st)

        def combine(e=p, es=4, x=p, xs=4, coef=_ptr(z), nv=2, t=_ptr(o), ts=4, ns=1):
            return getattr(L, 'emg3d_dev_sensitivity_combine_block' + sp)(4, 1, e, es, ns, x, xs, 1, coef, nv, t, ts, st)
        bad = {'sensitivity_dots_block': (dots, [dict(e=None), dict(x=None), dict(w=None), dict(out=None), dict(ws=None),
                                                 dict(nv=0), dict(nv=-3), dict(ns=0), dict(es=3), dict(xs=3), dict(wst=3),
                                                 dict(ws_len=need - 1)]),
               'sensitivity_combine_block': (combine, [dict(e=None), dict(x=None), dict(coef=None), dict(t=None), dict(nv=0),
                                                       dict(nv=-3), dict(ns=0), dict(es=3), dict(xs=3), dict(ts=3)])}
        for name, (call, cases) in bad.items():
            for kw in cases:
                assert call(**kw) == -1, (name, sp, kw)
                with pytest.raises(_lib.Emg3dAmdError, match=f"{name}: "):
                    _lib.check(call(**kw), 'emg3d_dev_' + name + sp)
        torch.cuda.synchronize()
        assert float(o.abs().sum()) == 0.0 and float(d.abs().sum()) == 0.0
        for name, (call, _) in bad.items():
            _lib.check(call(), 'emg3d_dev_' + name + sp)
        torch.cuda.synchronize()


# ----------------------------------------------------------------- methods on the gpu ---
K = 5
FREQS2 = {'f1': 1.0, 'f2': 2.5}
CASES = dict(ADJOINT_CASES)
CASES['two-frequencies'] = dict(case='VTI', mapping='Conductivity', freqs=FREQS2)
PASSES = [2, 8]


def _instance(name, **kw):
    spec = CASES[name]
    grid, model = small_model(spec['case'], spec['mapping'])
    if spec.get('comp'):
        kw['grids'] = _comp_grid()
    rec = gradient.ReciprocalSensitivity(model, SRCS, spec.get('freqs', FREQS), RECS, solver_opts=OPTS, tol_gradient=TOL,
                                         magnetic=spec.get('magnetic'), **kw)
    return grid, model, rec


def _vectors_and_data(name, rec, grid):
    """K random model vectors and K data sets: column 1 has NaN, column 2 lacks a pair, column 3 is empty."""
    rng = np.random.default_rng(23)
    V = rng.standard_normal((K, gradient._NCOMP[CASES[name]['case']]) + tuple(grid.shape_cells))
    Y = [_random_data(rng, rec.pairs, len(RECS)) for _ in range(K)]
    Y[1][rec.pairs[0]][1] = np.nan
    Y[1][rec.pairs[-1]][0] = np.nan
    del Y[2][rec.pairs[0]]
    Y[3] = {}
    W = {p: rng.uniform(0.1, 2.0, len(RECS)) for p in rec.pairs}
    W[rec.pairs[0]][2] = np.nan
    return V, Y, W


@functools.lru_cache(maxsize=None)
def _reference(name):
    """One case, once: the instance after ``forward()``, the inputs, and the K single-vector products of each kind."""
    grid, model, rec = _instance(name)
    V, Y, W = _vectors_and_data(name, rec, grid)
    ref = dict(jv=[rec.jvec(v) for v in V], jt=[rec.jtvec(y) for y in Y], hv=[rec.hessian_vec(v) for v in V],
               hw=[rec.hessian_vec(v, W) for v in V])
    return grid, model, rec, V, Y, W, ref


def _block_maxdiff(block, singles):
    """Largest difference of the slices of a block to the K single results, relative to the max-norm of these."""
    return float(np.max(np.abs(block - np.stack(singles))) / np.max(np.abs(np.stack(singles))))


@pytest.mark.gpu
@pytest.mark.parametrize('kc', PASSES)
@pytest.mark.parametrize('name', list(CASES))
def test_block_methods_equal_the_single_products(name, kc):
    """``jvec_block`` within 1e-10 of the max-norm of ``jvec`` per pair (reordered sums); ``jtvec_block`` the BITS of
    ``jtvec`` per column (columns with NaN, without a pair and without any datum are among them); adjointness per column
    to 1e-12 of the sum of the magnitudes of the terms of ``Re sum conj(y) jvec_block(v)``; ``hessian_vec_block`` within
    1e-10 of ``hessian_vec``, with and without weights. No product solves anything."""
    grid, model, rec, V, Y, W, ref = _reference(name)
    solves = dict(rec.n_solves)
    jv = rec.jvec_block(V, columns_per_pass=kc)
    jt = rec.jtvec_block(Y, columns_per_pass=kc)
    hv, hw = rec.hessian_vec_block(V, columns_per_pass=kc), rec.hessian_vec_block(V, W, columns_per_pass=kc)
    assert list(jv) == rec.pairs and all(jv[p].shape == (K, len(RECS)) and np.iscomplexobj(jv[p]) for p in rec.pairs)
    dv = max(float(np.max(np.abs(jv[p] - np.stack([r[p] for r in ref['jv']]))) /
                   np.max(np.abs(np.stack([r[p] for r in ref['jv']])))) for p in rec.pairs)
    same = all(np.array_equal(jt[k], ref['jt'][k]) for k in range(K))
    assert jt.shape == (K,) + ref['jt'][0].shape == hv.shape == hw.shape and jt.dtype == np.float64
    worst = 0.0
    for k in range(K):
        lhs = float(np.sum(V[k].reshape(jt[k].shape) * jt[k]))
        terms = np.concatenate([np.nan_to_num(np.conj(Y[k][p]) * jv[p][k]) for p in Y[k]] or [np.zeros(1)])
        rhs, mag = float(np.sum(terms.real)), float(np.sum(np.abs(terms)))
        if mag > 0:
            worst = max(worst, abs(lhs - rhs) / mag)
        else:
            assert lhs == 0.0
    dh, dw = _block_maxdiff(hv, ref['hv']), _block_maxdiff(hw, ref['hw'])
    record(f"block methods, {name}, columns_per_pass={kc}: jvec_block vs jvec {dv:.2e} (bound 1e-10); jtvec_block "
           f"bit-identical to jtvec: {same}; adjointness per column {worst:.2e} (bound 1e-12); hessian_vec_block vs "
           f"hessian_vec {dh:.2e}, weighted {dw:.2e} (bound 1e-10)")
    assert dv <= 1e-10
    assert same
    assert worst <= 1e-12
    assert dh <= 1e-10 and dw <= 1e-10
    assert rec.n_solves == solves and solves['jvec'] == solves['jtvec'] == 0


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_device_blocks(name):
    """``from_device(to_device(V)) == V``; the device route of ``hessian_vec_block`` (block in, block out) equals its
    NumPy route bit for bit, and so does ``jtvec_block(on_device=True)``; ``jvec_block`` of a device block equals that of
    the NumPy block; a block on the device, but wrong, is refused."""
    import torch
    grid, model, rec, V, Y, W, ref = _reference(name)
    B = rec.to_device(V)
    n = gradient._NCOMP[CASES[name]['case']]
    assert B.dtype == torch.float64 and B.shape == (K, n, grid.n_cells) and B.is_contiguous() and B.device == _dev()
    back = rec.from_device(B)
    assert back.shape == (K,) + ref['jt'][0].shape and np.array_equal(back, V.reshape(back.shape))
    assert all(back[k].flags['F_CONTIGUOUS'] for k in range(K))
    if n == 1:
        assert torch.equal(rec.to_device(V[:, 0]), B)                      # (K, nx, ny, nz) is accepted as well
    H = rec.hessian_vec_block(B, W)
    assert isinstance(H, torch.Tensor) and H.shape == B.shape and H.device == B.device
    assert np.array_equal(rec.from_device(H), rec.hessian_vec_block(V, W))
    assert np.array_equal(rec.hessian_vec_block(B, W, on_device=False), rec.from_device(H))
    assert torch.equal(rec.hessian_vec_block(V, W, on_device=True), H)
    T = rec.jtvec_block(Y, on_device=True)
    assert isinstance(T, torch.Tensor) and np.array_equal(rec.from_device(T), rec.jtvec_block(Y))
    ja, jb = rec.jvec_block(B), rec.jvec_block(V)
    assert all(np.array_equal(ja[p], jb[p]) for p in rec.pairs)
    for bad in (B.to(torch.float32), B[:, :, :-1], B.permute(0, 2, 1), B.reshape(K, -1)):
        with pytest.raises(ValueError, match="a device block must be"):
            rec.jvec_block(bad)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_host_kept_and_single_stored_fields(name):
    """``keep='host'`` and ``field_dtype='single'``: ``jtvec_block`` is the bits of their own ``jtvec`` per column,
    ``jvec_block`` within 1e-10 of their own ``jvec``; 'host' equals 'device' bit for bit in all three block products
    (the same kernels on the same bits); across the two storage types the block products differ by at most 1e-6 of the
    max-norm (2^-24 per kept value)."""
    grid, model, dev, V, Y, W, ref = _reference(name)
    got = {}
    for label, kw in (('host', dict(keep='host')), ('single', dict(field_dtype='single')),
                      ('single on the host', dict(keep='host', field_dtype='single'))):
        _, _, rec = _instance(name, **kw)
        jv, jt, hw = rec.jvec_block(V, columns_per_pass=2), rec.jtvec_block(Y, columns_per_pass=2), rec.hessian_vec_block(V, W)
        got[label] = (jv, jt, hw)
        own_jt = [rec.jtvec(y) for y in Y]
        own_jv = [rec.jvec(v) for v in V]
        same = all(np.array_equal(jt[k], own_jt[k]) for k in range(K))
        dv = max(float(np.max(np.abs(jv[p] - np.stack([r[p] for r in own_jv]))) /
                       np.max(np.abs(np.stack([r[p] for r in own_jv])))) for p in rec.pairs)
        record(f"block methods, {name}, {label}: jtvec_block bit-identical to its jtvec: {same}; jvec_block vs its jvec {dv:.2e} "
               f"(bound 1e-10)")
        assert same and dv <= 1e-10
        assert rec.n_solves == dev.n_solves
        rec.release()
    want = (dev.jvec_block(V, columns_per_pass=2), dev.jtvec_block(Y, columns_per_pass=2), dev.hessian_vec_block(V, W))
    for a, b in (('host', want), ('single on the host', got['single'])):
        same = (all(np.array_equal(got[a][0][p], b[0][p]) for p in dev.pairs) and np.array_equal(got[a][1], b[1]) and
                np.array_equal(got[a][2], b[2]))
        record(f"block methods, {name}, {a} vs keep='device': bit-identical: {same}")
        assert same
    diffs = (_maxdiff(got['single'][0], want[0]), _maxdiff(got['single'][1], want[1]), _maxdiff(got['single'][2], want[2]))
    record(f"block methods, {name}, single vs double: jvec_block {diffs[0]:.2e}, jtvec_block {diffs[1]:.2e}, hessian_vec_block "
           f"{diffs[2]:.2e} (max-norm relative, bound 1e-6)")
    assert max(diffs) <= 1e-6


@pytest.mark.gpu
def test_scratch_is_checked_against_free_memory(monkeypatch):
    """The scratch of a pass is compared with the free HBM before it is allocated: ``MemoryError`` naming
    ``columns_per_pass``."""
    import torch
    grid, model, rec, V, Y, W, ref = _reference('isotropic-resistivity')
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a, **k: (0, 1))
    monkeypatch.setattr(torch.cuda, 'memory_reserved', lambda *a, **k: 0)
    monkeypatch.setattr(torch.cuda, 'memory_allocated', lambda *a, **k: 0)
    for call in (lambda: rec.jvec_block(V), lambda: rec.jtvec_block(Y), lambda: rec.hessian_vec_block(V)):
        with pytest.raises(MemoryError, match="columns_per_pass"):
            call()
