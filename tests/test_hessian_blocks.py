"""The cell blocks of the Gauss-Newton Hessian and block-Jacobi: the kernel
``emg3d_dev_hessian_cell_blocks`` of ``csrc/hessian_blocks.h`` through the C ABI against NumPy, the method
``gradient.ReciprocalSensitivity.hessian_cell_blocks`` against the existing ``jtvec`` / ``hessian_diagonal`` /
``hessian_vec`` of the same object, the kernels ``emg3d_dev_pcg_update_blk`` / ``_direction_blk`` of ``csrc/pcg_block.h``
against NumPy in ``longdouble``, and ``gauss_newton_solve(precondition='block')`` against dense matrices.

Every criterion is derived, not tuned.

The kernel. ``Z_p = sum_{d: row[d] = p} Z_d`` are the pair sums of ``test_hessian_diagonal`` and ``S_p`` the same sums of
magnitudes. Per cell and packed row (p, q) the base is ``B_pq = f sum_{s,r} W S_p S_q``, ``f = scale (V / 4)^2``, and

    |got - want| <= (ns nr + 48) eps B_pq

for ANY order of summation, by the argument of ``test_hessian_diagonal``: each of the two (at most twelve-term) complex
sums is off by at most 16 eps S, so ``Re(conj(Z_p) Z_q)`` by 32 eps S_p S_q and a few more eps for the product and the
real part (the diagonal's 48 eps cover it with 14 to spare), and ns nr eps for the outer sum taken over the absolute
terms ``W S_p S_q``. ``h`` starts from random values of magnitude <= B_pq / 2; the rounding of that last addition stays
inside what the terms above leave unused, as there. With the exact rows ``B*`` Cauchy-Schwarz gives ``B*_pq^2 <= B*_pp
B*_qq``, and the same inequality on the sums of magnitudes ``B_pq^2 <= B_pp B_qq`` for the bases, hence for what the kernel
returns ``|got_pq| <= sqrt(B*_pp B*_qq) + c sqrt(B_pp B_qq) <= sqrt((B*_pp + c B_pp) (B*_qq + c B_qq))``, c = (ns nr + 48)
eps: the check ``got_pq^2 <= (B*_pp + bound_pp) (B*_qq + bound_qq)`` with the NumPy rows in the place of ``B*``.
The first n rows against ``emg3d_dev_hessian_diagonal``: within the sum of the two bounds always; for n <= 2 the tile (4 x
4) and every operation with its order are those of the diagonal kernel, and the rows must agree bit for bit. For n = 3 the
tile is 4 sources x 2 receivers: PAIRS still hold a full and a ragged tile either way (6 = 4 + 2 sources; 7 = 3 x 2 + 1
receivers).

The method. ``jtvec`` of unit data 1 and 1j gives the rows ``Re J_i`` and ``Im J_i`` (times the chain factors), so entry
[p, q] is ``sum_i w_i (Jre_i[p] Jre_i[q] + Jim_i[p] Jim_i[q])``; both sides round and read the same kept fields: twice
the bound times ``|chain_p chain_q|``. ``hessian_vec`` of the unit vector at (q, c) touches twelve edges: three bounds, as
for the diagonal.

The PCG kernels. A cell's ``A = B_c + lambda diag(rd_c)`` is built as ``G G^T`` plus a diagonal so that cond_2(A) <= 1e3,
which NumPy verifies (with positive definiteness) from the reference alone. The kernel forms A (one rounding per
diagonal entry: ``|dA| <= u |A|``, u = eps / 2), factorises it by Cholesky and solves by two substitutions: the computed z
satisfies ``(A + dA) z = r`` with ``|dA| <= gamma_{3n+1} |L^||L^T^|`` (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., Theorem 10.4) and ``|| |L^||L^T^| ||_2 <= n (1 - n gamma_{n+1})^-1 ||A||_2`` (its eq. 10.7): in all
``||dA||_2 <= (n (3n + 1) + 1) u ||A||_2`` to first order, so ``||z - z*||_2 <= cond_2(A) (n (3n + 1) + 1) u ||z*||_2`` and
with ``||.||_inf <= ||.||_2 <= sqrt(n) ||.||_inf``

    |z - z*|_inf <= c n cond_2(A) eps |z*|_inf,   c = (3n + 1 + 1 / n) sqrt(n) / 2 <= 9   (n = 3: 8.95; n = 2: 5.31).

C_CHOL = 9 is used for both n. Cells that take the fallback (planted: not definite, or all zero with rd = 0) follow the
Jacobi rule ``r / (hd + lambda rd)``, or r: one rounding for the sum, one for the quotient -- 2 eps -- and the decision
(no positive pivot) must be the reference's. Vector updates: 4 eps of the magnitudes, sums ``(N + 16) eps sum |terms|``,
both as in ``test_gauss_newton_solve``; where z enters, its own bound is added.

The solve. The two criteria of ``test_gauss_newton_solve._check_solution``; ``maxit`` is twice the iterations of a dense
CG with the exact block-Jacobi preconditioner (the n x n cell blocks of the dense matrix itself) plus 10.
"""
import functools

import numpy as np
import pytest

from emg3d_amd import _lib, gradient
from test_gauss_newton_solve import KC, LD, REG, ZERO, _check_solution, _dense, _from_model, _padded, _to_model
from test_gauss_newton_solve import TOL as SOLVE_TOL
from test_hessian_diagonal import METHOD_CASES, ROW_MAPS, _weights, pair_sums
from test_reciprocal import _comp_grid, _dev, _stack, _up
from test_sensitivity import EPS, FREQS, MU_0, OPTS, RECS, SRCS, TOL, _stretched, record, small_model

SYMBOLS = ('emg3d_dev_hessian_cell_blocks', 'emg3d_dev_hessian_cell_blocks_sp', 'emg3d_dev_pcg_update_blk',
           'emg3d_dev_pcg_direction_blk')
C_CHOL = 9


def packed_rows(n):
    """(p, q) of the packed rows: the diagonal first, then (0,1), (0,2), (1,2)."""
    return [(p, p) for p in range(n)] + [(p, q) for q in range(1, n) for p in range(q)]


# ----------------------------------------------------------------------- not gpu tests ---
def test_declared_symbols_and_method():
    header = open(_lib.HEADER).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name) and name + '(' in header
    assert _lib.SIGNATURES['emg3d_dev_hessian_cell_blocks'] == _lib.SIGNATURES['emg3d_dev_hessian_diagonal']
    assert _lib.SIGNATURES['emg3d_dev_hessian_cell_blocks_sp'] == _lib.SIGNATURES['emg3d_dev_hessian_diagonal']
    assert callable(gradient.ReciprocalSensitivity.hessian_cell_blocks)
    assert not hasattr(gradient.Sensitivity, 'hessian_cell_blocks')        # no receiver fields: no such method
    assert packed_rows(3) == gradient.ReciprocalSensitivity._packed_rows(3) == [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]


def test_weights_are_validated_and_another_grid_is_refused_before_any_gpu_work():
    grid, model = small_model('VTI', 'Conductivity')
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    rhs = np.ones((2,) + tuple(grid.shape_cells))
    bad = {'shape': {('a', 'f'): np.ones(len(RECS) + 1)}, 'scalar': {('b', 'f'): 1.0},
           'complex': {('a', 'f'): np.ones(len(RECS), dtype=complex)}, 'negative': {('a', 'f'): np.array([1., -1e-300, 2.])}}
    for what, w in bad.items():
        with pytest.raises(ValueError, match=r"`weights\[\('[ab]', 'f'\)\]` must"):
            rec.hessian_cell_blocks(w)
        with pytest.raises(ValueError, match=r"`weights\[\('[ab]', 'f'\)\]` must"):
            rec.gauss_newton_solve(rhs, [1.0], weights=w, precondition='block')
    assert rec.n_solves == ZERO and rec.kept_bytes == 0
    for grids in (_comp_grid(), {('b', 'f'): _comp_grid(), ('a', 'f'): _comp_grid()}):
        rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, grids=grids)
        with pytest.raises(NotImplementedError, match="hessian_cell_blocks: .*`grids`"):
            rec.hessian_cell_blocks()
        with pytest.raises(NotImplementedError, match=r"gauss_newton_solve\(precondition='block'\): .*`grids`"):
            rec.gauss_newton_solve(rhs, [1.0, 2.0], precondition='block')
        assert rec.n_solves == ZERO and rec.kept_bytes == 0


def test_no_cpu_fallback_without_gpu():
    if _lib.lib().emg3d_device_count() > 0:
        pytest.skip("GPU present")
    grid, model = small_model('VTI', 'Conductivity')
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.hessian_cell_blocks()
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        rec.gauss_newton_solve(np.ones((2,) + tuple(grid.shape_cells)), [1.0], precondition='block')


# ------------------------------------------------------------------------ the checker ---
def blocks_and_bound(Z, S, W, rows, scale, vol3):
    """``f sum_{s,r} W Re(conj(Z_p) Z_q)`` per packed row (p, q) and cell, (n (n + 1) / 2, nx, ny, nz), and the same
    with the sums of magnitudes ``S`` in the place of ``Z``: the bases B_pq of the module docstring."""
    f = scale * (vol3 / 4) ** 2
    n = max(rows) + 1
    z, s = ([sum(A[d] for d in range(3) if rows[d] == p) for p in range(n)] for A in (Z, S))
    want = np.stack([f * np.sum(W * np.real(np.conj(z[p]) * z[q]), axis=(-2, -1)) for p, q in packed_rows(n)])
    B = np.stack([f * np.sum(W * s[p] * s[q], axis=(-2, -1)) for p, q in packed_rows(n)])
    return want, B


# ------------------------------------------------------------------- kernel on the gpu ---
# a workgroup owns 16 x 4 x 4 cells: (67, 5, 9) and (19, 6, 7) exceed that along every axis by a ragged remainder; tiles
# of 4 x 4 (n <= 2) or 4 x 2 (n = 3) sources x receivers: (6, 7) is a full and a ragged tile either way for both
SHAPES = [(1, 1, 1), (5, 3, 2), (67, 5, 9), (19, 6, 7)]
PAIRS = [(1, 1), (3, 5), (6, 7)]


@functools.lru_cache(maxsize=2)
def _kernel_inputs(shape, ns, nr, is_complex, single=False):
    """Stacks (NaN-padded, on the device; ``single``: rounded to single precision, the checker gets the rounded values),
    volumes, weights with exact zeros, and the checker's Z and S: once for the four row maps."""
    grid = _stretched(*shape)
    rng = np.random.default_rng(2000 * sum(shape) + 10 * ns + nr + is_complex)
    (E, es), (X, xs) = _stack(rng, ns, grid.n_edges, is_complex), _stack(rng, nr, grid.n_edges, is_complex)
    if single:
        narrow = np.complex64 if is_complex else np.float32
        E, X = E.astype(narrow), X.astype(narrow)
    W = rng.uniform(0.1, 2.0, (ns, nr))
    W[rng.random((ns, nr)) < 0.3] = 0.0
    vol = grid.cell_volumes.astype(np.float64)
    n = grid.n_edges
    wide = complex if is_complex else float
    Ew, Xw = E[:, :n].astype(wide), X[:, :n].astype(wide)
    Z, S = pair_sums(Ew, Xw, shape), pair_sums(np.abs(Ew), np.abs(Xw), shape)
    return dict(E=_up(E), es=es, X=_up(X), xs=xs, W=W, Wd=_up(W), vol=_up(vol), vol3=vol.reshape(shape, order='F'), Z=Z, S=S)


def _call(name, inp, shape, ns, nr, is_complex, rows, scale, start, hs):
    from emg3d_amd._device import _ptr, _stream
    h = _up(start)
    _lib.check(getattr(_lib.lib(), name)(
        *shape, int(is_complex), _ptr(inp['E']), inp['es'], ns, _ptr(inp['X']), inp['xs'], nr, _ptr(inp['Wd']), *rows, scale,
        _ptr(inp['vol']), _ptr(h), hs, _stream()), name)
    return h.cpu().numpy().reshape(-1, hs)


def _check_kernel(tag, name, shape, ns, nr, is_complex, case, single=False):
    rows = ROW_MAPS[case]
    inp = _kernel_inputs(shape, ns, nr, is_complex, single)
    ncell, n = int(np.prod(shape)), max(rows) + 1
    npack = n * (n + 1) // 2
    scale = 0.37
    contribution, B = blocks_and_bound(inp['Z'], inp['S'], inp['W'], rows, scale, inp['vol3'])
    rng = np.random.default_rng(7 + len(case))
    h0 = np.where(B > 0, rng.uniform(-0.5, 0.5, B.shape) * B, rng.standard_normal(B.shape))
    hs = ncell + 5
    start = np.full((npack, hs), np.nan)
    start[:, :ncell] = np.stack([r.ravel('F') for r in h0])
    got = _call(name, inp, shape, ns, nr, is_complex, rows, scale, start, hs)
    assert got.shape == (npack, hs)
    assert np.all(np.isnan(got[:, ncell:])) and not np.any(np.isnan(got[:, :ncell]))
    got3 = np.stack([r.reshape(shape, order='F') for r in got[:, :ncell]])
    bound = (ns * nr + 48) * EPS * B
    diff = np.abs(got3 - (h0 + contribution))
    worst = float(np.max(diff[B > 0] / bound[B > 0])) if np.any(B > 0) else 0.0
    record(f"{tag} {shape} ns={ns} nr={nr} complex={is_complex} {case}: max |diff| / bound = {worst:.2e} "
           f"(bound (ns nr + 48) eps B_pq); entries with B = 0: {int(np.sum(B == 0))}")
    assert np.all(diff <= bound)
    again = _call(name, inp, shape, ns, nr, is_complex, rows, scale, start, hs)
    assert np.array_equal(got, again, equal_nan=True)
    return inp, rows, n, contribution, bound, start, got, hs, scale


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(ROW_MAPS))
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('ns, nr', PAIRS)
@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_vs_numpy(shape, ns, nr, is_complex, case):
    """The bound of the module docstring per cell and packed row; ``h`` starts from random values and has NaN behind each
    row, which must survive; a second call gives the same bits. The first n rows against ``emg3d_dev_hessian_diagonal``
    from the same start: within the sum of the two bounds, and bit for bit for n <= 2 (same tile, same order). From
    zeros: Cauchy-Schwarz per cell."""
    name = 'emg3d_dev_hessian_cell_blocks'
    inp, rows, n, contribution, bound, start, got, hs, scale = _check_kernel('hessian_cell_blocks', name, shape, ns, nr,
                                                                             is_complex, case)
    ncell = int(np.prod(shape))
    diag = _call('emg3d_dev_hessian_diagonal', inp, shape, ns, nr, is_complex, rows, scale, start[:n], hs)
    flat = np.stack([b.ravel('F') for b in bound])
    assert np.all(np.abs(got[:n, :ncell] - diag[:, :ncell]) <= 2 * flat[:n])
    same = np.array_equal(got[:n, :ncell], diag[:, :ncell])
    record(f"hessian_cell_blocks {shape} ns={ns} nr={nr} complex={is_complex} {case}: diagonal rows have the bits of "
           f"hessian_diagonal: {same}")
    if n <= 2:
        assert same
    zeros = np.where(np.isnan(start), np.nan, 0.0)
    rows0 = _call(name, inp, shape, ns, nr, is_complex, rows, scale, zeros, hs)[:, :ncell]
    exact = np.stack([c.ravel('F') for c in contribution])
    for m, (p, q) in enumerate(packed_rows(n)):
        if p != q:
            assert np.all(rows0[m] ** 2 <= (exact[p] + flat[p]) * (exact[q] + flat[q]))


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['isotropic', 'VTI', 'triaxial'])
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('ns, nr', PAIRS)
@pytest.mark.parametrize('shape', [(5, 3, 2), (19, 6, 7)])
def test_kernel_sp_vs_numpy(shape, ns, nr, is_complex, case):
    """Stacks stored in single precision: the same checker fed the rounded values, the same bound."""
    _check_kernel('hessian_cell_blocks_sp', 'emg3d_dev_hessian_cell_blocks_sp', shape, ns, nr, is_complex, case, single=True)


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    """Every one of them with ``EMG3D_ERR_BADARG`` (-1) before anything is launched: those of ``hessian_diagonal``, and a
    row map that leaves a row below the largest empty. n = 1 is accepted."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    a = torch.zeros(64, dtype=torch.complex128, device=_dev())             # a 2 x 2 x 2 grid: 54 edges, 8 cells
    w, vol, d = (torch.zeros(n, dtype=torch.float64, device=_dev()) for n in (1, 8, 48))   # h: six rows of 8 cells
    p, st = _ptr(a), _stream()
    good = dict(nx=2, ny=2, nz=2, c=1, e=p, es=54, ns=1, x=p, xs=54, nr=1, w=_ptr(w), rx=0, ry=1, rz=2, scale=1.0,
                vol=_ptr(vol), h=_ptr(d), hs=8)

    def call(**kw):
        k = {**good, **kw}
        return L.emg3d_dev_hessian_cell_blocks(k['nx'], k['ny'], k['nz'], k['c'], k['e'], k['es'], k['ns'], k['x'], k['xs'],
                                               k['nr'], k['w'], k['rx'], k['ry'], k['rz'], k['scale'], k['vol'], k['h'],
                                               k['hs'], st)
    bad = [dict(e=None), dict(x=None), dict(w=None), dict(vol=None), dict(h=None), dict(nx=0), dict(ny=0), dict(nz=-1),
           dict(ns=0), dict(nr=0), dict(es=53), dict(xs=53), dict(rx=3), dict(ry=-1), dict(rz=3), dict(hs=7),
           dict(rx=0, ry=2, rz=2), dict(rx=1, ry=1, rz=1), dict(rx=2, ry=0, rz=2),       # an empty row below the largest
           dict(nx=1, ny=4 * 65535 + 1, nz=1, es=10 ** 8, xs=10 ** 8, hs=10 ** 8),       # more than 65 535 workgroups along y
           dict(nx=1, ny=1, nz=4 * 65535 + 1, es=10 ** 8, xs=10 ** 8, hs=10 ** 8)]
    for kw in bad:
        assert call(**kw) == -1, kw
        with pytest.raises(_lib.Emg3dAmdError, match="hessian_cell_blocks: "):
            _lib.check(call(**kw), 'emg3d_dev_hessian_cell_blocks')
    torch.cuda.synchronize()
    assert float(d.abs().sum()) == 0.0 and float(a.abs().sum()) == 0.0
    for kw in (dict(), dict(rx=0, ry=0, rz=0), dict(rx=1, ry=0, rz=1)):     # triaxial, n = 1, n = 2
        _lib.check(call(**kw), 'emg3d_dev_hessian_cell_blocks')


# -------------------------------------------------------------------- method on the gpu ---
CASES = ['HTI', 'VTI', 'triaxial-LgResistivity', 'isotropic-resistivity', 'magnetic-receiver', 'laplace']


@functools.lru_cache(maxsize=None)
def _method(name):
    """One case, once: the object, the weights, ``hessian_cell_blocks``, the same from ``jtvec`` of unit data, the bound
    of the module docstring times |chain_p chain_q| per entry, ``hessian_diagonal``, and the solve counts."""
    spec = METHOD_CASES[name]
    grid, model = small_model(spec['case'], spec['mapping'])
    freqs = spec.get('freqs', FREQS)
    rec = gradient.ReciprocalSensitivity(model, SRCS, freqs, RECS, solver_opts=OPTS, tol_gradient=TOL,
                                         magnetic=spec.get('magnetic'))
    rec.forward()
    before = dict(rec.n_solves)
    w = _weights(np.random.default_rng(71))
    Bk = rec.hessian_cell_blocks(w)
    after = dict(rec.n_solves)
    n, shape = gradient._NCOMP[spec['case']], tuple(grid.shape_cells)
    is_complex = freqs['f'] > 0
    W = np.stack([np.nan_to_num(w.get(p, np.zeros(len(RECS)))) for p in rec.pairs])
    rowwise = np.zeros((n, n) + shape)
    for s, pair in enumerate(rec.pairs):
        for r in range(len(RECS)):
            if W[s, r] > 0:
                unit = np.zeros(len(RECS), dtype=complex)
                unit[r] = 1.0
                for y in ([unit, 1j * unit] if is_complex else [unit]):
                    J = rec.jtvec({pair: y}).reshape((n,) + shape)
                    rowwise += W[s, r] * J[:, None] * J[None, :]
    E, X = (t.cpu().numpy() for t in rec._stacks['f'])
    smu0 = 2j * np.pi * freqs['f'] * MU_0 if is_complex else -freqs['f'] * MU_0
    S = pair_sums(np.abs(E), np.abs(X), shape)
    _, B = blocks_and_bound(S, S, W, ROW_MAPS[spec['case']], abs(smu0) ** 2, grid.cell_volumes.reshape(shape, order='F'))
    chain = np.stack([gradient._DCHAIN[spec['mapping']](np.ones(shape), np.asarray(getattr(model, prop), dtype=float))
                      for prop in gradient._PROPS[spec['case']]])
    bound = np.zeros((n, n) + shape)
    for m, (p, q) in enumerate(packed_rows(n)):
        bound[p, q] = bound[q, p] = (len(SRCS) * len(RECS) + 48) * EPS * B[m] * np.abs(chain[p] * chain[q])
    H = rec.hessian_diagonal(w).reshape((n,) + shape)
    return dict(grid=grid, model=model, rec=rec, w=w, Bk=Bk, rowwise=rowwise, bound=bound, H=H, before=before, after=after,
                n=n, shape=shape, freqs=freqs)


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_method_equals_the_row_by_row_route(name):
    """Every entry against the rows of ``jtvec`` within twice its bound; the diagonal against ``hessian_diagonal`` within
    the sum of the two bounds; symmetric bit for bit; the device result round-trips; no solve."""
    m = _method(name)
    Bk, rowwise, bound, rec, n, shape = m['Bk'], m['rowwise'], m['bound'], m['rec'], m['n'], m['shape']
    assert Bk.shape == (n, n) + shape and Bk.dtype == np.float64
    assert np.all(bound > 0)
    worst = float(np.max(np.abs(Bk - rowwise) / (2 * bound)))
    record(f"hessian_cell_blocks vs row by row, {name}: max |diff| / (2 bound) = {worst:.2e}; n_solves {m['before']} -> "
           f"{m['after']}")
    assert m['before'] == m['after'] == {'forward': 2, 'receiver': 3, 'jvec': 0, 'jtvec': 0}
    assert np.all(np.abs(Bk - rowwise) <= 2 * bound)
    diag = np.stack([Bk[p, p] for p in range(n)])
    dbound = np.stack([bound[p, p] for p in range(n)])
    worst = float(np.max(np.abs(diag - m['H']) / (2 * dbound)))
    record(f"hessian_cell_blocks diagonal vs hessian_diagonal, {name}: max |diff| / (2 bound) = {worst:.2e}; the same bits: "
           f"{np.array_equal(diag, m['H'])}")
    assert np.all(np.abs(diag - m['H']) <= 2 * dbound)
    for p in range(n):
        for q in range(p):
            assert np.array_equal(Bk[p, q], Bk[q, p])
    before = dict(rec.n_solves)
    packed = rec.hessian_cell_blocks(m['w'], on_device=True)
    ncell = int(np.prod(shape))
    assert tuple(packed.shape) == (n * (n + 1) // 2, ncell) and str(packed.dtype) == 'torch.float64' and packed.is_cuda
    host = packed.cpu().numpy()
    for k, (p, q) in enumerate(packed_rows(n)):
        assert np.array_equal(host[k].reshape(shape, order='F'), Bk[p, q])
    assert rec.n_solves == before


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['HTI', 'triaxial-LgResistivity'])
def test_hessian_vec_of_a_unit_vector_gives_a_column_of_the_block(name):
    """``hessian_vec(unit vector at (q, c), w)[p, c] == hessian_cell_blocks(w)[p, q, c]`` for every p within three times
    the bound, at the six cells of ``test_hessian_diagonal``'s unit-vector test."""
    m = _method(name)
    rec, Bk, bound, n, shape = m['rec'], m['Bk'], m['bound'], m['n'], m['shape']
    before = dict(rec.n_solves)
    cells = [(0, 0, 0), (9, 9, 7), (9, 0, 7), (0, 9, 0), (4, 5, 3), (6, 2, 5)]
    worst = 0.0
    for k, cell in enumerate(cells):
        q = k % n
        v = np.zeros((n,) + shape)
        v[(q,) + cell] = 1.0
        hv = rec.hessian_vec(v, m['w'])
        for p in range(n):
            c = (p, q) + cell
            worst = max(worst, abs(hv[(p,) + cell] - Bk[c]) / (3 * bound[c]))
            assert abs(hv[(p,) + cell] - Bk[c]) <= 3 * bound[c], (c, hv[(p,) + cell], Bk[c], bound[c])
    record(f"hessian_vec(unit at (q, c))[p, c] vs hessian_cell_blocks[p, q, c], {name}: max |diff| / (3 bound) = {worst:.2e} "
           f"over {len(cells)} cells")
    assert rec.n_solves == before


@pytest.mark.gpu
def test_host_kept_fields_and_default_weights():
    """``keep='host'`` gives the bits of ``keep='device'``; ``weights=None`` the bits of all-ones weights; no weights at
    all: zeros."""
    m = _method('VTI')
    host = gradient.ReciprocalSensitivity(m['model'], SRCS, FREQS, RECS, solver_opts=OPTS, tol_gradient=TOL, keep='host')
    assert np.array_equal(host.hessian_cell_blocks(m['w']), m['Bk'])
    assert host.n_solves == {'forward': 2, 'receiver': 3, 'jvec': 0, 'jtvec': 0}
    host.release()
    rec = m['rec']
    ones = {pair: np.ones(len(RECS)) for pair in rec.pairs}
    B1 = rec.hessian_cell_blocks()
    assert np.array_equal(B1, rec.hessian_cell_blocks(ones)) and not np.array_equal(B1, m['Bk'])
    assert np.array_equal(rec.hessian_cell_blocks({}), np.zeros(B1.shape))
    corr = np.abs(B1[0, 1]) / np.sqrt(B1[0, 0] * B1[1, 1])
    record(f"hessian_cell_blocks VTI small survey: |B_01| / sqrt(B_00 B_11) median {float(np.median(corr)):.3f}, max "
           f"{float(np.max(corr)):.3f}")


# --------------------------------------------------------------- PCG kernels on the gpu ---
def _blk_inputs(rng, ncell, n, ncol, rd_rows):
    """Packed blocks, diag R ((ncell,) or (n, ncell)), dampings, mask, and the planted cells (``bad``: B_01^2 > B_00 B_11
    with rd = 0 -- not definite; ``zero``: the whole block and rd are 0)."""
    G = rng.standard_normal((ncell, n, n))
    F2 = np.sum(G * G, axis=(1, 2))
    delta = F2 / 500
    B = G @ np.swapaxes(G, 1, 2) + delta[:, None, None] * np.eye(n)
    rd = rng.uniform(0.1, 1.0, (n, ncell) if rd_rows else (ncell,)) * delta
    lam = 10 ** rng.uniform(-1, 1, ncol)
    act = rng.uniform(size=ncell) < 0.8 if ncell > 1 else np.array([True])
    pick = rng.permutation(ncell)
    bad, zero = (pick[:max(1, ncell // 50)], pick[max(1, ncell // 50):2 * max(1, ncell // 50)]) if ncell > 1 else ([], [])
    for c in bad:
        B[c, 0, 1] = B[c, 1, 0] = 2 * np.sqrt(B[c, 0, 0] * B[c, 1, 1])
    B[zero] = 0.0
    rd[..., bad] = 0.0
    rd[..., zero] = 0.0
    kind = np.zeros(ncell, dtype=int)
    kind[bad], kind[zero] = 1, 2
    packed = np.stack([B[:, p, q] for p, q in packed_rows(n)])
    return B, packed, rd, lam, act, kind


def _z_model(r, B, rd, lam, act, kind, n):
    """(z* (n, ncell) in longdouble, its bound per element, cond_2(A)) for one column: ``A^-1 r`` on the regular cells -- which the
    reference alone shows positive definite with cond_2 <= 1e3 --, the Jacobi rule on the planted ones."""
    ncell = r.shape[1]
    rdn = np.broadcast_to(rd, (n, ncell))
    A = B + lam * np.einsum('kc,kl->ckl', rdn, np.eye(n))
    ev = np.linalg.eigvalsh(A)
    reg = kind == 0
    assert np.all(ev[reg, 0] > 0) and np.all(ev[reg, -1] / ev[reg, 0] <= 1e3)
    assert np.all(ev[kind == 1, 0] < 0) and np.all(ev[kind == 2] == 0)
    cond = np.where(reg, ev[:, -1] / np.where(reg, ev[:, 0], 1.0), 1.0)
    z = np.zeros((n, ncell), dtype=LD)
    z[:, reg] = np.linalg.solve(A[reg], r.T[reg][:, :, None])[:, :, 0].T
    res = np.einsum('ckl,lc->kc', A[reg].astype(LD), z[:, reg]) - r[:, reg]       # one step of refinement in longdouble
    z[:, reg] -= np.linalg.solve(A[reg], np.asarray(res, dtype=float).T[:, :, None])[:, :, 0].T
    d = np.stack([B[:, k, k] for k in range(n)]).astype(LD) + LD(lam) * rdn
    jac = np.where(d > 0, r.astype(LD) / np.where(d > 0, d, 1), r.astype(LD))
    z[:, ~reg] = jac[:, ~reg]
    zinf = np.max(np.abs(z), axis=0)
    bound = np.where(reg, C_CHOL * n * cond * EPS * zinf, 2 * EPS * np.abs(z))
    z[:, ~act], bound = 0, np.where(act, bound, 0.0)
    return z, np.asarray(bound, dtype=float), cond


def _blk(ncell, n, K, first, x, r, p, q, packed, rd, rds, mask, table, pq, tol, hbs=None):
    """update_blk -> scalar -> direction_blk on copies of the host arrays; (x, r, p, table) as NumPy. The rows of the
    blocks are ``hbs`` apart with NaN between them."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    hbs = ncell + 3 if hbs is None else hbs
    hb = np.full((len(packed), hbs), np.nan)
    hb[:, :ncell] = packed
    xd, rdv, pd, qd, hbd, rdd = (_padded(a) for a in (x, r, p, q, hb, rd))
    md = None if mask is None else _up(mask.astype(np.uint8))
    td, pqd = _up(table), _padded(pq)
    ws_len = L.emg3d_pcg_ws_len(ncell, K)
    ws = torch.full((ws_len,), float('nan'), dtype=torch.float64, device=_dev())
    diag = (_ptr(hbd), hbs, _ptr(rdd), rds, None if md is None else _ptr(md))
    _lib.check(L.emg3d_dev_pcg_update_blk(ncell, n, K, first, _ptr(xd), _ptr(rdv), _ptr(pd), _ptr(qd), *diag, _ptr(td), _ptr(pqd),
                                          _ptr(ws), ws_len, _stream()), 'emg3d_dev_pcg_update_blk')
    _lib.check(L.emg3d_dev_pcg_scalar(ncell, K, first, tol, _ptr(td), _ptr(pqd), _ptr(ws), ws_len, _stream()),
               'emg3d_dev_pcg_scalar')
    _lib.check(L.emg3d_dev_pcg_direction_blk(ncell, n, K, first, _ptr(pd), _ptr(rdv), *diag, _ptr(td), _stream()),
               'emg3d_dev_pcg_direction_blk')
    N = K * n * ncell
    out = [a.cpu().numpy() for a in (xd, rdv, pd)]
    assert all(np.all(np.isnan(a[N:])) for a in out)
    return out[0][:N], out[1][:N], out[2][:N], td.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('rd_rows', [False, True], ids=['rd-shared', 'rd-rows'])
@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('n', [2, 3])
@pytest.mark.parametrize('ncell', [1, 255, 257, 1024 * 256 + 257])
def test_pcg_block_kernels_vs_numpy(ncell, n, K, rd_rows):
    """The set-up (``first`` = 1: p = z, which shows z) and one ordinary step against the model of the module docstring,
    with a mask, different dampings per column and (K = 3) column 1 frozen: its x, r, p keep their bits."""
    rng = np.random.default_rng(ncell + 11 * n + 5 * K + rd_rows)
    B, packed, rd, lams, act, kind = _blk_inputs(rng, ncell, n, K, rd_rows)
    rds = ncell if rd_rows else 0
    N = n * ncell
    tol = 1e-3
    # ---- the set-up: r holds b; z through p
    b = rng.standard_normal((K, n, ncell))
    first = np.zeros((K, 8))
    first[:, 0] = lams
    if K == 3:
        first[1, 7] = 1.0
    nan = np.full_like(b, np.nan)
    fx, fr, fp, ft = _blk(ncell, n, K, 1, nan, b, nan, nan, packed, rd, rds, act, first, np.full(K, np.nan), tol)
    fr, fp = fr.reshape(K, n, ncell), fp.reshape(K, n, ncell)
    worst_z = worst_sum = 0.0
    for k in range(K):
        if K == 3 and k == 1:
            assert np.array_equal(fr[k], b[k]) and np.all(np.isnan(fp[k])) and np.array_equal(ft[k], first[k])
            continue
        assert np.array_equal(fr[k], np.where(act, b[k], 0.0))
        z, zb, cond = _z_model(fr[k], B, rd, lams[k], act, kind, n)
        err = np.abs(fp[k] - z).astype(float)
        some = zb > 0
        worst_z = max(worst_z, float(np.max(err[some] / zb[some], initial=0.0)))
        assert np.all(err <= zb), (k, worst_z)
        assert np.all(fp[k][:, ~act] == 0.0)
        plain = (kind == 2) & act
        assert np.array_equal(fp[k][:, plain], fr[k][:, plain])                   # all zero, rd = 0: the identity
        rz, rr = np.sum(fr[k] * z), np.sum(fr[k].astype(LD) ** 2)
        brz = (N + 16) * EPS * np.sum(np.abs(fr[k] * z)) + np.sum(np.abs(fr[k]) * zb)
        assert abs(ft[k, 5] - rr) <= (N + 16) * EPS * rr and ft[k, 1] == ft[k, 5] and ft[k, 6] == 0
        assert abs(ft[k, 2] - rz) <= brz
        worst_sum = max(worst_sum, float(abs(ft[k, 2] - rz) / brz), float(abs(ft[k, 5] - rr) / ((N + 16) * EPS * rr)))
    # ---- an ordinary step
    x, r, p, q = rng.standard_normal((4, K, n, ncell))
    table = np.zeros((K, 8))
    table[:, 0] = lams
    table[:, 1] = N                                        # <b,b>: nothing converges (<r,r> is about N)
    table[:, 2] = rng.uniform(0.5, 2.0, K)
    table[:, 6] = 4
    if K == 3:
        table[1, 7] = 1.0
    pq = rng.uniform(0.5, 2.0, K) * 50
    got = _blk(ncell, n, K, 0, x, r, p, q, packed, rd, rds, act, table, pq, tol)
    gx, gr, gp = (a.reshape(K, n, ncell) for a in got[:3])
    gt = got[3]
    for k in range(K):
        if K == 3 and k == 1:
            assert np.array_equal(gx[k], x[k]) and np.array_equal(gr[k], r[k]) and np.array_equal(gp[k], p[k])
            assert np.array_equal(gt[k], table[k])
            continue
        alpha = table[k, 2] / pq[k]
        assert np.all(np.abs(gx[k] - (x[k] + LD(alpha) * p[k])) <= 4 * EPS * (np.abs(x[k]) + np.abs(alpha * p[k])))
        want_r = np.where(act, r[k] - LD(alpha) * q[k], 0)
        assert np.all(np.abs(gr[k] - want_r) <= 4 * EPS * (np.abs(r[k]) + np.abs(alpha * q[k])))
        assert np.all(gr[k][:, ~act] == 0.0)
        z, zb, cond = _z_model(gr[k], B, rd, lams[k], act, kind, n)
        rz, rr = np.sum(gr[k] * z), np.sum(gr[k].astype(LD) ** 2)
        brz = (N + 16) * EPS * np.sum(np.abs(gr[k] * z)) + np.sum(np.abs(gr[k]) * zb)
        assert abs(gt[k, 2] - rz) <= brz and abs(gt[k, 5] - rr) <= (N + 16) * EPS * rr
        worst_sum = max(worst_sum, float(abs(gt[k, 2] - rz) / brz), float(abs(gt[k, 5] - rr) / ((N + 16) * EPS * rr)))
        assert gt[k, 3] == table[k, 2] and gt[k, 4] == pq[k] and gt[k, 6] == 5 and gt[k, 7] == 0
        beta = gt[k, 2] / gt[k, 3]
        assert np.all(np.abs(gp[k] - (z + LD(beta) * p[k])) <= zb + 4 * EPS * (np.abs(z) + np.abs(beta * p[k])))
    again = _blk(ncell, n, K, 0, x, r, p, q, packed, rd, rds, act, table, pq, tol)
    assert all(np.array_equal(a, c) for a, c in zip(got, again))
    record(f"pcg block kernels n_cells={ncell} n={n} K={K} rd rows={rd_rows}: max |z - z*|_inf / bound = {worst_z:.2e} "
           f"(bound {C_CHOL} n cond eps |z*|_inf), sums max |diff| / bound = {worst_sum:.2e}")


@pytest.mark.gpu
def test_pcg_block_bad_arguments_are_refused():
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    ncell = 8
    v, hb, rd, t, pq = (torch.zeros(k, dtype=torch.float64, device=_dev()) for k in (2 * ncell, 3 * ncell, ncell, 8, 1))
    ws_len = L.emg3d_pcg_ws_len(ncell, 1)
    ws = torch.zeros(ws_len, dtype=torch.float64, device=_dev())
    x, r, p, q = (v.clone() for _ in range(4))
    good = dict(vpc=2, hb=_ptr(hb), hbs=ncell, rd=_ptr(rd), rds=0)

    def update(**kw):
        k = {**good, **kw}
        return L.emg3d_dev_pcg_update_blk(ncell, k['vpc'], 1, 0, _ptr(x), _ptr(r), _ptr(p), _ptr(q), k['hb'], k['hbs'], k['rd'],
                                          k['rds'], None, _ptr(t), _ptr(pq), _ptr(ws), ws_len, _stream())

    def direction(**kw):
        k = {**good, **kw}
        return L.emg3d_dev_pcg_direction_blk(ncell, k['vpc'], 1, 0, _ptr(p), _ptr(r), k['hb'], k['hbs'], k['rd'], k['rds'], None,
                                             _ptr(t), _stream())
    for kw in (dict(vpc=1), dict(vpc=4), dict(hb=None), dict(rd=None), dict(hbs=ncell - 1), dict(rds=ncell - 1)):
        for call, what in ((update, 'pcg_update_blk: '), (direction, 'pcg_direction_blk: ')):
            assert call(**kw) == -1, kw
            with pytest.raises(_lib.Emg3dAmdError, match=what):
                _lib.check(call(**kw), what)
    pq.fill_(1.0)
    t[2] = 1.0
    _lib.check(update(), 'emg3d_dev_pcg_update_blk')
    _lib.check(direction(), 'emg3d_dev_pcg_direction_blk')
    torch.cuda.synchronize()


# -------------------------------------------------------------------- solve on the gpu ---
def _block_cg_numpy(A, b, n, tol, maxit=5000):
    """Dense CG with the exact block-Jacobi preconditioner, the n x n cell blocks of ``A`` itself (the unknowns of cell c
    are c, c + n_cells, ...): the iterations to ``|r| <= tol |b|``."""
    ncell = len(A) // n
    idx = np.arange(ncell)[:, None] + ncell * np.arange(n)[None, :]
    blocks = A[idx[:, :, None], idx[:, None, :]]

    def M(r):
        z = np.empty_like(r)
        z[idx] = np.linalg.solve(blocks, r[idx][:, :, None])[:, :, 0]
        return z
    x, r = np.zeros_like(b), b.copy()
    z = M(r)
    p, rz = z.copy(), r @ z
    for it in range(1, maxit + 1):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        if np.linalg.norm(r) <= tol * np.linalg.norm(b):
            return it
        z = M(r)
        rz, old = r @ z, rz
        p = z + rz / old * p
    raise AssertionError("the dense reference's own CG did not converge")


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['VTI', 'triaxial'])
def test_block_solve_vs_dense(name):
    """``precondition='block'`` reaches the dense solution for three dampings under the two criteria of
    ``_check_solution``; the result does not depend on ``check_every``, bit for bit; iteration counts beside Jacobi's are
    recorded."""
    grid, rec, active, act, lams, b, dense = _dense(name)
    n = gradient._NCOMP[rec.model.case]
    before = dict(rec.n_solves)
    its = [_block_cg_numpy(A, bk[act], n, SOLVE_TOL) for (A, *_), bk in zip(dense, b)]
    maxit = 2 * max(its) + 10
    rhs = _to_model(rec, grid, b)
    x, info = rec.gauss_newton_solve(rhs, lams, tol=SOLVE_TOL, maxit=maxit, precondition='block', columns_per_pass=KC, **REG)
    assert x.shape == (3, n) + tuple(grid.shape_cells)
    assert set(info) == {'iterations', 'relative_residual', 'state', 'history', 'hessian_passes', 'preconditioner_passes',
                         'data_rank'}
    assert info['preconditioner_passes'] == 0 and info['data_rank'] is None
    _check_solution(f"{name} precondition='block'", dense, _from_model(x), info, act, b)
    x3, info3 = rec.gauss_newton_solve(rhs, lams, tol=SOLVE_TOL, maxit=maxit, precondition='block', check_every=3,
                                       columns_per_pass=KC, **REG)
    x1, info1 = rec.gauss_newton_solve(rhs, lams, tol=SOLVE_TOL, maxit=maxit, precondition='block', check_every=1,
                                       columns_per_pass=KC, **REG)
    assert np.array_equal(x, x3) and np.array_equal(x, x1)
    assert np.array_equal(info['iterations'], info3['iterations']) and np.array_equal(info['iterations'], info1['iterations'])
    jmax = 2 * max(d[3] for d in dense) + 10
    _, jac = rec.gauss_newton_solve(rhs, lams, tol=SOLVE_TOL, maxit=jmax, columns_per_pass=KC, **REG)
    record(f"gauss_newton_solve {name} to tol {SOLVE_TOL}: iterations Jacobi {jac['iterations'].tolist()} (dense CG "
           f"{[d[3] for d in dense]}), block {info['iterations'].tolist()} (dense CG {its})")
    assert rec.n_solves == before


@pytest.mark.gpu
def test_one_component_takes_the_jacobi_route():
    """Isotropic: ``'block'`` gives the bits of ``True``, through the same entry points."""
    grid, rec, active, act, lams, b, dense = _dense('isotropic')
    maxit = 2 * max(d[3] for d in dense) + 10
    rhs = _to_model(rec, grid, b)
    x, info = rec.gauss_newton_solve(rhs, lams, tol=SOLVE_TOL, maxit=maxit, **REG)
    xb, infob = rec.gauss_newton_solve(rhs, lams, tol=SOLVE_TOL, maxit=maxit, precondition='block', **REG)
    assert np.array_equal(x, xb) and np.array_equal(info['iterations'], infob['iterations'])
    assert np.array_equal(info['relative_residual'], infob['relative_residual'])
    dev = _dev()
    w = rec._check_weights(None)
    geo = rec._regulariser_geometry(None, dev)
    alphas = rec._check_regulariser(REG['smallness'], REG['smoothness'])
    pcgs = [rec._pcg(dev, rec.to_device(rhs), lams, KC, w, geo, alphas, None, route) for route in (True, 'block')]
    assert pcgs[0]._update[0] == pcgs[1]._update[0] == 'emg3d_dev_pcg_update'
    assert pcgs[0]._direction[0] == pcgs[1]._direction[0] == 'emg3d_dev_pcg_direction'


def _one_shot_solve(rec, rhs, lams, route, maxit, tol, kc):
    """The loop of ``gauss_newton_solve`` with every product over the kept fields a one-shot call on a fresh pass:
    (x as NumPy, the ``_BlockPCG``)."""
    dev = _dev()
    w = rec._check_weights(None)
    geo = rec._regulariser_geometry(None, dev)
    alphas = rec._check_regulariser(REG['smallness'], REG['smoothness'])
    lam = rec._check_dampings(lams)
    K = len(lam)
    pcg = rec._pcg(dev, rec.to_device(rhs).clone(), lam, kc, w, geo, alphas, None, route, None, tol)
    pcg.step(1)
    for it in range(maxit):
        if not np.any(pcg.table.cpu().numpy()[:, 7] == 0):
            break
        q = rec.hessian_vec_block(pcg.p, None, on_device=True, columns_per_pass=kc)
        rec._regulariser(geo, alphas, pcg.p, q, beta=1.0, lam=pcg.lam, pq=pcg.pq, ws=pcg.rws, irls=None)
        pcg.ps = rec._pass(dev, K, kc, w)                  # the preconditioner of 'data' applies on a fresh pass too
        pcg.step(0, q)
    return rec.from_device(pcg.x), pcg


@pytest.mark.gpu
@pytest.mark.parametrize('route', [True, False, 'data'], ids=['jacobi', 'none', 'data'])
def test_the_other_preconditioners_keep_their_calls_and_bits(route):
    """``True``, ``False`` and ``'data'`` on the VTI survey: the entry points they went through before there was a fourth
    variant, Jacobi from the bits of ``hessian_diagonal``, and the bits of the same iteration made of one-shot calls."""
    import torch
    grid, rec, active, act, lams, b, dense = _dense('VTI')
    rhs = _to_model(rec, grid, b)
    maxit, tol = 12, 1e-6
    x, info = rec.gauss_newton_solve(rhs, lams, tol=tol, maxit=maxit, precondition=route, check_every=5,
                                     columns_per_pass=KC, **REG)
    want, pcg = _one_shot_solve(rec, rhs, lams, route, maxit, tol, KC)
    assert np.array_equal(x, want) and float(np.abs(x).max()) > 0
    assert np.array_equal(info['iterations'], pcg.table.cpu().numpy()[:, 6].astype(int))
    assert pcg._update[0] == 'emg3d_dev_pcg_update'
    assert pcg._direction[0] == ('emg3d_dev_pcg_direction_z' if route == 'data' else 'emg3d_dev_pcg_direction')
    hd, rd, mask = pcg.held
    if route is True:
        assert torch.equal(hd, rec.to_device(rec.hessian_diagonal()[None])[0]) and tuple(rd.shape) == (grid.n_cells,)
    else:
        assert hd is None and rd is None
    assert (pcg.pre is not None) == (route == 'data')
