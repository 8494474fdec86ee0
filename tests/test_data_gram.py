"""Data-space Gauss-Newton matrix without solves: the kernel ``emg3d_dev_data_gram`` of
``csrc/gram.h`` through the C ABI against NumPy written out in this file, and
``gradient.ReciprocalSensitivity.data_gram`` / ``stack_data`` / ``unstack_data`` against the existing ``jtvec`` /
``jvec`` of the same object.

The criterion of every comparison is derived, not tuned. With the pairs' sums of magnitudes
``S_{i,p}(c) = sum_{d: row[d] = p} sum_{k in E_d(c)} |e_s[k]| |x_r[k]|`` (i = (s, r)) and

    B_ij = sum_{p,c} mw[p, c] (V_c / 4)^2 |scale_a| |scale_b| S^A_{i,p}(c) S^B_{j,p}(c),

    |got - want| <= (nrows n_cells + C) eps B_ij,        C = 40,

holds for ANY order of summation (eps = 2^-52, twice the unit roundoff u; nrows: property rows). Per factor a^ of a
term: each real component of the twelve-term complex sum Z is a sum of 24 real products in fused multiply-adds,
error <= 24 u S = 12 eps S per component; ``scale * Z`` mixes the components, (|Re scale| + |Im scale|) 12 eps S <=
17 eps |scale| S, and rounds twice itself, 2 u |scale| |Z| <= 1 eps |scale| S; the weight ``sqrt(mw) V / 4`` that
either factor carries rounds in the root (<= 1 ulp = 1 eps) and in the product (u; V / 4 is exact), and its product
with the component rounds once more (u): 17 + 1 + 1 + 1 = 20 eps relative to the factor's magnitude bound, 40 eps for
the product of two factors. The sum of the nrows n_cells terms (cells of ragged patches add exact zeros, and the
merging of partial sums is part of the same summation tree) rounds at most once per term on the way to the root:
nrows n_cells u per unit of sum |terms| <= B -- counted in eps, which leaves the second-order terms a factor of two.

Inputs, the small survey and the recorder come from ``test_sensitivity``, the device helpers and the NaN-padded stacks
from ``test_reciprocal``, the pair sums from ``test_hessian_diagonal``.
"""
import functools

import numpy as np
import pytest

from emg3d_amd import _lib, gradient
from test_hessian_diagonal import ROW_MAPS, pair_sums
from test_reciprocal import _comp_grid, _dev, _stack, _up
from test_sensitivity import ADJOINT_CASES, EPS, MU_0, OPTS, RECS, SRCS, TOL, _stretched, record, small_model

C_BOUND = 40                       # the C of the module docstring
FREQS2 = {'f': 1.0, 'g': 2.5}
LAPLACE2 = {'f': -1.0, 'g': -2.5}
NAMES = ('emg3d_data_gram_ws_len', 'emg3d_dev_data_gram')


# ----------------------------------------------------------------------- not gpu tests ---
def test_declared_symbols_and_methods():
    header = open(_lib.HEADER).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name) and name + '(' in header
    for method in ('data_gram', 'stack_data', 'unstack_data'):
        assert callable(getattr(gradient.ReciprocalSensitivity, method))
        assert not hasattr(gradient.Sensitivity, method)                  # no receiver fields: no such method
    L = _lib.lib()
    assert L.emg3d_data_gram_ws_len(0, 1, 1, 1, 1, 1) == 0 and L.emg3d_data_gram_ws_len(1, 1, 1, 1, 1, 0) == 0
    assert L.emg3d_data_gram_ws_len(1, 1, 1, 1, 1, 1) >= 64 * 64 and L.emg3d_data_gram_ws_len(1, 1, 1, 0, 1, 1) >= 32 * 32


def test_stack_and_unstack_data():
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS2, RECS)
    nrec, npairs = len(RECS), len(rec.pairs)
    N = npairs * nrec
    rng = np.random.default_rng(5)
    y = {p: rng.standard_normal(nrec) + 1j * rng.standard_normal(nrec) for p in rec.pairs}
    v = rec.stack_data(y)
    assert v.shape == (2 * N,) and v.dtype == np.float64
    for k, pair in enumerate(rec.pairs):                                   # the ordering, entry by entry
        for r in range(nrec):
            assert v[k * nrec + r] == y[pair][r].real and v[N + k * nrec + r] == y[pair][r].imag
    back = rec.unstack_data(v)
    assert list(back) == list(rec.pairs) and all(np.array_equal(back[p], y[p]) and np.iscomplexobj(back[p]) for p in y)
    assert np.array_equal(rec.stack_data(back), v)
    # NaN and a missing pair: 0
    holes = {p: a.copy() for p, a in y.items()}
    gone = rec.pairs[2]
    del holes[gone]
    holes[rec.pairs[0]][1] = np.nan
    holes[rec.pairs[1]][2] = complex(1.0, np.nan)
    want = v.copy()
    for k, r in ((0, 1), (1, 2)):
        want[k * nrec + r] = want[N + k * nrec + r] = 0.0
    want[2 * nrec:3 * nrec] = want[N + 2 * nrec:N + 3 * nrec] = 0.0
    got = rec.stack_data(holes)
    assert np.array_equal(got, want) and not np.isnan(got).any()
    assert np.array_equal(rec.stack_data({}), np.zeros(2 * N))
    # wrong lengths
    with pytest.raises(ValueError, match=r"`vector\[\('a', 'f'\)\]` must have shape"):
        rec.stack_data({('a', 'f'): np.ones(nrec + 1)})
    for bad in (np.ones(2 * N + 1), np.ones(N), np.ones((2 * N, 1)), np.ones(2 * N, dtype=complex)):
        with pytest.raises(ValueError, match="`vector` must be real with shape"):
            rec.unstack_data(bad)
    # a Laplace-domain survey: M = N, real values
    lap = gradient.ReciprocalSensitivity(model, SRCS, LAPLACE2, RECS)
    yl = {p: rng.standard_normal(nrec) for p in lap.pairs}
    vl = lap.stack_data(yl)
    assert vl.shape == (N,) and np.array_equal(vl, np.concatenate([yl[p] for p in lap.pairs]))
    bl = lap.unstack_data(vl)
    assert all(np.array_equal(bl[p], yl[p]) and not np.iscomplexobj(bl[p]) for p in yl)
    with pytest.raises(ValueError, match="`vector` must be real with shape"):
        lap.unstack_data(np.ones(2 * N))
    for obj in (rec, lap):                                                 # nothing touched the GPU
        assert obj.n_solves == {'forward': 0, 'receiver': 0, 'jvec': 0, 'jtvec': 0} and obj.kept_bytes == 0


def test_arguments_are_validated_before_any_gpu_work():
    grid, model = small_model()
    shape = tuple(grid.shape_cells)
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS2, RECS)
    tiny = np.ones(shape)
    tiny[3, 2, 1] = -1e-300
    bad = {'shape': np.ones(shape[:2]), 'rows': np.ones((2,) + shape), 'complex': np.ones(shape, dtype=complex),
           'negative': -np.ones(shape), 'barely negative': tiny, 'nan': np.full(shape, np.nan)}
    for what, m in bad.items():
        with pytest.raises(ValueError, match="`model_weights` must be"):
            rec.data_gram(m)
    assert rec.n_solves == {'forward': 0, 'receiver': 0, 'jvec': 0, 'jtvec': 0} and rec.kept_bytes == 0
    pairs = [(s, f) for s in SRCS for f in FREQS2]
    for grids in (_comp_grid(), {p: _comp_grid() for p in pairs}):
        other = gradient.ReciprocalSensitivity(model, SRCS, FREQS2, RECS, grids=grids)
        with pytest.raises(NotImplementedError, match="`grids`"):
            other.data_gram()
        assert other.n_solves['forward'] == 0 and other.kept_bytes == 0
    mixed = gradient.ReciprocalSensitivity(model, SRCS, {'f': 1.0, 'l': -1.0}, RECS)
    for call in (mixed.data_gram, lambda: mixed.stack_data({}), lambda: mixed.unstack_data(np.zeros(12))):
        with pytest.raises(NotImplementedError, match="mixes Laplace- and frequency-domain"):
            call()
    assert mixed.n_solves['forward'] == 0 and mixed.kept_bytes == 0


def test_no_cpu_fallback_without_gpu():
    if _lib.lib().emg3d_device_count() > 0:
        pytest.skip("GPU present")
    grid, model = small_model()
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS2, RECS)
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.data_gram()


# ------------------------------------------------------------------- kernel on the gpu ---
# A workgroup owns a patch of 16 x 2 x 2 cells at a time and a pair of tiles of 4 sources x 8 receivers; a launch has
# at most 256 workgroups per pair of tiles.
#   (1, 1, 1): one cell; (5, 2, 2): inside one patch; (19, 5, 3): 2 x 3 x 2 patches, a ragged remainder along every
#   axis; (35, 23, 15): 3 x 12 x 8 = 288 patches > 256 workgroups -- the grid-stride loop runs twice for 32 of them
#   and the second launch adds 256 partial tiles.
#   (1, 1): one datum; (3, 5): one ragged tile (and ragged 4 x 2 sub-blocks of it); (6, 7): two tiles, the second
#   with 2 of 4 sources, both with 7 of 8 receivers -- a symmetric block of 2 x 2 tile pairs, one of them mirrored;
#   (2, 9): two tiles along the receivers, the second with one receiver.
SCALE_A, SCALE_B = complex(0.3, -1.1), complex(-0.7, 0.45)
BIG = (35, 23, 15)
KERNEL_CASES = [(shape, a, a) for shape in [(1, 1, 1), (5, 2, 2), (19, 5, 3)] for a in [(1, 1), (3, 5), (6, 7)]]
KERNEL_CASES += [((19, 5, 3), (3, 5), (2, 9)), ((19, 5, 3), (6, 7), (1, 1)), ((5, 2, 2), (2, 9), (6, 7))]
KERNEL_PARAMS = [c + (is_complex, case) for c in KERNEL_CASES for is_complex in (True, False) for case in ROW_MAPS]
# the large grid: the NumPy side is the cost, so few data and one map per kind of field
KERNEL_PARAMS += [(BIG, (2, 3), (2, 3), True, 'VTI'), (BIG, (2, 3), (2, 3), False, 'triaxial'),
                  (BIG, (2, 3), (1, 2), True, 'triaxial'), (BIG, (2, 3), (1, 2), False, 'isotropic')]


@functools.lru_cache(maxsize=4)
def _side(shape, ns, nr, is_complex, seed):
    """One side's stacks (host, NaN-padded, and device) and the checker's pair sums Z and sums of magnitudes S, as
    [d] -> (n_cells, ns * nr); cells in C order of (nx, ny, nz) -- any order serves, the same for all cell arrays."""
    grid = _stretched(*shape)
    n = grid.n_edges
    rng = np.random.default_rng(seed + 1000 * sum(shape) + 10 * ns + nr + is_complex)
    (E, es), (X, xs) = _stack(rng, ns, n, is_complex), _stack(rng, nr, n, is_complex)
    Z = [z.reshape(-1, ns * nr) for z in pair_sums(E[:, :n], X[:, :n], shape)]
    S = [s.reshape(-1, ns * nr) for s in pair_sums(np.abs(E[:, :n]), np.abs(X[:, :n]), shape)]
    return dict(E=_up(E), es=es, X=_up(X), xs=xs, Z=Z, S=S, ns=ns, nr=nr)


def _panels(side, rows, scale, is_complex):
    """(J, Smag): per property row p the rows a^ of the module docstring, (nrows, c n, n_cells) in longdouble, and their
    magnitude bounds |scale| S (the same for the real and the imaginary half)."""
    J, Sm = [], []
    for p in range(max(rows) + 1):
        z = scale * sum(side['Z'][d] for d in range(3) if rows[d] == p)
        s = abs(scale) * sum(side['S'][d] for d in range(3) if rows[d] == p)
        parts = [z.real, z.imag] if is_complex else [z.real]
        J.append(np.concatenate([q.T for q in parts]).astype(np.longdouble))
        Sm.append(np.concatenate([s.T] * len(parts)).astype(np.longdouble))
    return np.stack(J), np.stack(Sm)


def _gram_call(shape, is_complex, A, B, sa, sb, rows, mw, mws, vol, out, ld, ws=None):
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    ws_len = L.emg3d_data_gram_ws_len(*shape, int(is_complex), A['ns'] * A['nr'], B['ns'] * B['nr'])
    ws = torch.full((ws_len,), float('nan'), dtype=torch.float64, device=_dev())
    _lib.check(L.emg3d_dev_data_gram(
        *shape, int(is_complex), _ptr(A['E']), A['es'], A['ns'], _ptr(A['X']), A['xs'], A['nr'], sa.real, sa.imag,
        _ptr(B['E']), B['es'], B['ns'], _ptr(B['X']), B['xs'], B['nr'], sb.real, sb.imag, *rows, _ptr(mw), mws, _ptr(vol),
        _ptr(out), ld, _ptr(ws), ws_len, _stream()), 'emg3d_dev_data_gram')
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('shape, a, b, is_complex, case', KERNEL_PARAMS)
def test_kernel_vs_numpy(shape, a, b, is_complex, case):
    """The bound of the module docstring per entry; ``out`` starts as NaN with ``ld > cols`` -- the padding must
    survive, the block must be free of NaN --, the stacks and ``mw`` have NaN behind every row, ``mw`` has exact
    zeros; a second call gives the same bits; with the same side twice the block equals its transpose bit for bit."""
    rows = ROW_MAPS[case]
    same = a == b
    A = _side(shape, *a, is_complex, 1)
    B = A if same else _side(shape, *b, is_complex, 2)
    sa = SCALE_A if is_complex else complex(SCALE_A.real)
    sb = sa if same else SCALE_B if is_complex else complex(SCALE_B.real)
    c = 2 if is_complex else 1
    ncell, nrows = int(np.prod(shape)), max(rows) + 1
    vol = _stretched(*shape).cell_volumes.astype(np.float64).reshape(shape, order='F').ravel()   # C order, as the pair sums
    rng = np.random.default_rng(17 + len(case) + ncell)
    mw = rng.uniform(0.1, 2.0, (nrows, ncell))
    mw[rng.random((nrows, ncell)) < 0.3] = 0.0
    mw[:, 0] = 1.5
    # the kernel's cells are x fastest: hand it the Fortran-ordered arrays
    to_f = np.arange(ncell).reshape(shape).ravel(order='F')
    mws = ncell + 7
    mw_dev = np.full((nrows, mws), np.nan)
    mw_dev[:, :ncell] = mw[:, to_f]
    JA, SA = _panels(A, rows, sa, is_complex)
    JB, SB = (JA, SA) if same else _panels(B, rows, sb, is_complex)
    w = (mw * (vol / 4) ** 2).astype(np.longdouble)
    want = np.einsum('pic,pc,pjc->ij', JA, w, JB)
    Bnd = np.einsum('pic,pc,pjc->ij', SA, w, SB)
    bound = ((nrows * ncell + C_BOUND) * EPS * Bnd).astype(float)
    ma, mb = c * a[0] * a[1], c * b[0] * b[1]
    ld = mb + 3
    args = (shape, is_complex, A, B, sa, sb, rows, _up(mw_dev), mws, _up(vol[to_f]))
    got = _gram_call(*args, _up(np.full((ma, ld), np.nan)), ld)
    assert np.all(np.isnan(got[:, mb:])) and not np.any(np.isnan(got[:, :mb]))
    diff = np.abs(got[:, :mb] - want).astype(float)
    assert np.all(bound > 0)
    record(f"data_gram {shape} A={a} B={b} complex={is_complex} {case}: max |diff| / bound = "
           f"{float(np.max(diff / bound)):.2e} (bound ({nrows} * {ncell} + {C_BOUND}) eps B)")
    assert np.all(diff <= bound)
    again = _gram_call(*args, _up(np.full((ma, ld), np.nan)), ld)
    assert np.array_equal(got, again, equal_nan=True)
    if same:
        assert np.array_equal(got[:, :mb], got[:, :mb].T)


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    """Every one of them with ``EMG3D_ERR_BADARG`` (-1) and the prefix ``data_gram: `` before anything is launched."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    a = torch.zeros(64, dtype=torch.complex128, device=_dev())             # a 2 x 2 x 2 grid: 54 edges, 8 cells
    mw, vol, out = (torch.zeros(n, dtype=torch.float64, device=_dev()) for n in (24, 8, 4))
    ws_len = L.emg3d_data_gram_ws_len(2, 2, 2, 1, 1, 1)
    ws = torch.zeros(ws_len, dtype=torch.float64, device=_dev())
    p, st = _ptr(a), _stream()
    good = dict(nx=2, ny=2, nz=2, c=1, ea=p, esa=54, nsa=1, xa=p, xsa=54, nra=1, sar=1.0, sai=0.5, eb=p, esb=54, nsb=1,
                xb=p, xsb=54, nrb=1, sbr=1.0, sbi=0.5, rx=0, ry=1, rz=2, mw=_ptr(mw), mws=8, vol=_ptr(vol), out=_ptr(out),
                ld=2, ws=_ptr(ws), ws_len=ws_len)

    def call(**kw):
        k = {**good, **kw}
        return L.emg3d_dev_data_gram(*(k[name] for name in good), st)
    big = 10 ** 8
    bad = [dict(ea=None), dict(xa=None), dict(eb=None), dict(xb=None), dict(mw=None), dict(vol=None), dict(out=None),
           dict(ws=None), dict(nx=0), dict(ny=0), dict(nz=-1), dict(nsa=0), dict(nra=0), dict(nsb=0), dict(nrb=-2),
           dict(rx=3), dict(ry=-1), dict(rz=3), dict(esa=53), dict(xsa=53), dict(esb=53), dict(xsb=53), dict(mws=7),
           dict(ld=1), dict(ws_len=ws_len - 1), dict(ws_len=0),
           dict(nsa=4 * 256, nsb=4 * 257, ld=big, ws_len=10 ** 15),        # 256 x 257 > 65 535 pairs of tiles
           dict(nra=8 * 65535 + 1, ld=big, ws_len=10 ** 15)]
    for kw in bad:
        assert call(**kw) == -1, kw
        with pytest.raises(_lib.Emg3dAmdError, match="data_gram: "):
            _lib.check(call(**kw), 'emg3d_dev_data_gram')
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and float(ws.abs().sum()) == 0.0 and float(a.abs().sum()) == 0.0
    _lib.check(call(), 'emg3d_dev_data_gram')                               # (the good call is one)
    torch.cuda.synchronize()


# -------------------------------------------------------------------- method on the gpu ---
METHOD_CASES = {name: dict(ADJOINT_CASES[name], freqs=FREQS2) for name in (
    'isotropic-resistivity', 'HTI', 'VTI', 'triaxial-LgResistivity', 'magnetic-receiver')}
METHOD_CASES['laplace'] = dict(case='isotropic', mapping='Resistivity', freqs=LAPLACE2)
N_SOLVES = {'forward': 4, 'receiver': 6, 'jvec': 0, 'jtvec': 0}


def _unit_data(rec, k, r, value):
    y = np.zeros(len(RECS), dtype=complex)
    y[r] = value
    return {rec.pairs[k]: y}


@functools.lru_cache(maxsize=None)
def _method(name):
    """One case, once: the object, the model weights (random, with exact zeros), ``data_gram``, the same from 2 N
    calls of the existing ``jtvec``, the bound of the module docstring with ``mw = m chain^2`` per entry, and the solve
    counts before and after."""
    spec = METHOD_CASES[name]
    grid, model = small_model(spec['case'], spec['mapping'])
    freqs = spec['freqs']
    rec = gradient.ReciprocalSensitivity(model, SRCS, freqs, RECS, solver_opts=OPTS, tol_gradient=TOL,
                                         magnetic=spec.get('magnetic'))
    rec.forward()
    before = dict(rec.n_solves)
    shape = tuple(grid.shape_cells)
    nprop, nrec = gradient._NCOMP[spec['case']], len(RECS)
    rng = np.random.default_rng(83)
    m = rng.uniform(0.1, 2.0, (nprop,) + shape)
    m[rng.random(m.shape) < 0.2] = 0.0
    G = rec.data_gram(m if nprop > 1 else m[0])
    after = dict(rec.n_solves)
    is_complex = freqs['f'] > 0
    c = 2 if is_complex else 1
    N = len(rec.pairs) * nrec
    Jhat = np.zeros((c * N, m.size))
    for k in range(len(rec.pairs)):
        for r in range(nrec):
            Jhat[k * nrec + r] = rec.jtvec(_unit_data(rec, k, r, 1.0)).ravel()
            if is_complex:
                Jhat[N + k * nrec + r] = rec.jtvec(_unit_data(rec, k, r, 1j)).ravel()
    route = (Jhat * m.ravel()) @ Jhat.T
    # the bound: |s mu0| S per datum and property row, in the ordering of the matrix
    rows = ROW_MAPS[spec['case']]
    Smag = np.zeros((nprop, N, int(np.prod(shape))))
    for fname, mine, *_ in rec._per_frequency():
        E, X = (t.cpu().numpy() for t in rec._stacks[fname])
        smu0 = 2j * np.pi * freqs[fname] * MU_0 if is_complex else -freqs[fname] * MU_0
        S = [s.reshape(-1, len(mine), nrec) for s in pair_sums(np.abs(E), np.abs(X), shape)]
        for p in range(nprop):
            sp = abs(smu0) * sum(S[d] for d in range(3) if rows[d] == p)          # (n_cells, sources, receivers)
            for row, k in enumerate(mine):
                Smag[p, k * nrec:(k + 1) * nrec] = sp[:, row, :].T
    chain = np.stack([gradient._DCHAIN[spec['mapping']](np.ones(shape), np.asarray(getattr(model, prop), dtype=float))
                      for prop in gradient._PROPS[spec['case']]])
    w = (m * chain ** 2 * (grid.cell_volumes.reshape(shape, order='F') / 4) ** 2).reshape(nprop, -1)
    Smag = np.concatenate([Smag] * c, axis=1)
    bound = (nprop * Smag.shape[2] + C_BOUND) * EPS * np.einsum('pic,pc,pjc->ij', Smag, w, Smag)
    return dict(grid=grid, model=model, rec=rec, m=m if nprop > 1 else m[0], G=G, route=route, bound=bound, before=before,
                after=after, N=N, c=c)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(METHOD_CASES))
def test_method_equals_the_row_by_row_route(name):
    """``data_gram(m) == (Jhat * m) @ Jhat.T`` with the rows of ``Jhat`` from 2 N calls of ``jtvec`` (unit data and 1j
    times them; Laplace: N calls) within twice the bound -- both sides round, both read the same kept fields, so no
    solver tolerance enters. Two frequencies: the cross-frequency blocks are part of it."""
    d = _method(name)
    G, route, bound = d['G'], d['route'], d['bound']
    assert d['before'] == d['after'] == N_SOLVES
    assert G.shape == (d['c'] * d['N'],) * 2 and G.dtype == np.float64 and np.all(bound > 0)
    diff = np.abs(G - route)
    record(f"data_gram vs row by row, {name}: max |diff| / (2 bound) = {float(np.max(diff / (2 * bound))):.2e}; max "
           f"relative {float(np.max(diff) / np.max(np.abs(G))):.2e}; n_solves {d['before']} -> {d['after']}")
    assert np.all(diff <= 2 * bound)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['VTI', 'triaxial-LgResistivity', 'laplace'])
def test_matrix_times_data_is_jvec_of_jtvec(name):
    """``data_gram(m) @ stack_data(y) == sign * stack_data(jvec(m * jtvec(y)))`` for random y with one NaN and one
    missing pair (entries of magnitude <= 1 per part), within three times the bound summed over the row with the
    weights |stack_data(y)| (``dots`` adds twelve-term sums per edge).

    ``sign``: the rows of the matrix are those of ``jtvec`` (that makes it positive semi-definite), and ``jvec`` is the
    adjoint of ``jtvec`` up to the factor ``-1 / kappa``, ``kappa = conj(1 / -s mu0) * -s mu0`` the strength that a unit
    residual source carries (``jvec`` scales its sums by ``-s mu0 / kappa``, ``jtvec`` by ``s mu0``, gradient.py; the
    reference's residual source and gradient field do the same): +1 for the imaginary ``s mu0`` of the frequency domain,
    -1 for the real one of the Laplace domain. The test first asserts that premise on ``jvec`` and ``jtvec`` alone."""
    d = _method(name)
    rec = d['rec']
    sign = 1.0 if d['c'] == 2 else -1.0
    before = dict(rec.n_solves)
    rng = np.random.default_rng(89)
    y = {p: rng.uniform(-1, 1, len(RECS)) + (1j * rng.uniform(-1, 1, len(RECS)) if d['c'] == 2 else 0)
         for p in rec.pairs}
    del y[rec.pairs[1]]
    y[rec.pairs[2]][0] = np.nan
    ys = rec.stack_data(y)
    # the premise: sum(v * jtvec(y)) == sign * Re sum conj(y) jvec(v), both from the same kept fields
    v = rng.standard_normal(np.shape(d['m']))
    model_side = float(np.sum(v * rec.jtvec(y)))
    data_side = float(ys @ rec.stack_data(rec.jvec(v)))
    record(f"sum(v jtvec(y)) / Re sum(conj(y) jvec(v)), {name}: {model_side / data_side:+.12f} (premise: {sign:+.0f})")
    assert abs(model_side - sign * data_side) <= 1e-6 * abs(model_side)
    left = d['G'] @ ys
    right = sign * rec.stack_data(rec.jvec(d['m'] * rec.jtvec(y)))
    bound = 3 * d['bound'] @ np.abs(ys)
    diff = np.abs(left - right)
    record(f"data_gram @ y vs {sign:+.0f} * jvec(m jtvec(y)), {name}: max |diff| / (3 sum bound |y|) = "
           f"{float(np.max(diff / bound)):.2e}")
    assert rec.n_solves == before
    assert np.all(diff <= bound)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['HTI', 'laplace'])
def test_basic_properties(name):
    d = _method(name)
    rec, G, M = d['rec'], d['G'], d['c'] * d['N']
    assert G.shape == (M, M) and G.flags.c_contiguous and np.array_equal(G, G.T)
    assert np.linalg.eigvalsh(G)[0] >= -np.sum(np.diag(d['bound']))
    ones = rec.data_gram()
    assert np.array_equal(ones, rec.data_gram(np.ones(np.shape(d['m'])))) and not np.array_equal(ones, G)
    assert np.array_equal(ones, ones.T) and np.all(np.diag(ones) > 0)
    assert np.array_equal(rec.data_gram(np.zeros(np.shape(d['m']))), np.zeros((M, M)))
    assert np.array_equal(rec.data_gram(d['m']), G)                        # the same call: the same bits
    assert rec.n_solves == N_SOLVES


@pytest.mark.gpu
def test_host_kept_fields():
    """``keep='host'`` with two frequencies gives the bits of ``keep='device'``, and the second staging pair that the
    cross-frequency blocks need is gone after the call: a repeated call leaves the allocated HBM where it was."""
    import torch
    d = _method('VTI')
    host = gradient.ReciprocalSensitivity(d['model'], SRCS, FREQS2, RECS, solver_opts=OPTS, tol_gradient=TOL, keep='host')
    assert np.array_equal(host.data_gram(d['m']), d['G'])
    assert host.n_solves == N_SOLVES
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    again = host.data_gram(d['m'])
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and len(host._stage) == 2
    assert np.array_equal(again, d['G'])
    host.release()
