"""The data-space (Woodbury) preconditioner of ``gauss_newton_solve``: the kernels of
``csrc/precondition.h`` -- ``emg3d_dev_pcg_scale``, ``emg3d_dev_data_space_filter``, ``emg3d_dev_pcg_finish``,
``emg3d_dev_pcg_direction_z`` -- against NumPy in ``longdouble`` written out in this file, the preconditioner itself
(``ReciprocalSensitivity._data_preconditioner``) against dense inverses, and ``gauss_newton_solve(precondition='data')``
against dense solutions and dense models of its iteration counts.

Inputs, the small survey and the recorder come from ``test_sensitivity``, the device helpers from ``test_reciprocal``, the
dense systems and their checks from ``test_gauss_newton_solve``; figures that the GPU tests observe are printed and, with
``EMG3D_AMD_PARITY_FILE`` set, appended to that file.
"""
import functools

import numpy as np
import pytest

from emg3d_amd import _lib, gradient
from test_gauss_newton_solve import (KC, REG, TOL, ZERO, _check_solution, _columns, _dense, _from_model, _padded,
                                     _pcg_numpy, _survey, _to_model)
from test_reciprocal import _dev, _up
from test_sensitivity import EPS, FREQS, RECS, SRCS, record, small_model

SYMBOLS = ('emg3d_dev_pcg_scale', 'emg3d_data_space_filter_ws_len', 'emg3d_dev_data_space_filter', 'emg3d_dev_pcg_finish',
           'emg3d_dev_pcg_direction_z')
LD = np.longdouble
BADARG, SCRATCH = -1, -3
PCG_CAP = 1024 * 256                  # cells that the grid of the vector kernels covers in one round


# ----------------------------------------------------------------------- not gpu tests ---
def test_symbols_are_declared():
    header = open(_lib.HEADER).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name) and name + '(' in header
    assert any(s.endswith('precondition.h') for s in _lib.SOURCES)
    assert _lib.lib().emg3d_data_space_filter_ws_len(5, 3) == 15
    assert callable(gradient.ReciprocalSensitivity._data_preconditioner)


def test_arguments_are_validated_before_any_gpu_work():
    from test_reciprocal import _comp_grid
    grid, model = small_model()
    shape = tuple(grid.shape_cells)
    rec = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS)
    for bad in (0, -1, 2.5, True, 'all'):
        with pytest.raises(ValueError, match="`data_rank` must be") as err:
            rec.gauss_newton_solve(np.ones(shape), [1.0, 10.0], precondition='data', data_rank=bad)
        assert "Provided:" in str(err.value), bad
    assert rec.n_solves == ZERO and rec.kept_bytes == 0
    other = gradient.ReciprocalSensitivity(model, SRCS, FREQS, RECS, grids=_comp_grid())
    with pytest.raises(NotImplementedError) as a:
        other.data_gram()
    with pytest.raises(NotImplementedError) as b:
        other.gauss_newton_solve(np.ones(shape), [1.0], precondition='data')
    assert str(a.value).split(':', 1)[1] == str(b.value).split(':', 1)[1]
    assert other.n_solves == ZERO and other.kept_bytes == 0
    for freqs in ({'f': -1.0}, {'f': 1.0, 'g': -2.0}):
        laplace = gradient.ReciprocalSensitivity(model, SRCS, freqs, RECS)
        with pytest.raises(NotImplementedError):
            laplace.gauss_newton_solve(np.ones(shape), [1.0], precondition='data')
        assert laplace.n_solves == ZERO and laplace.kept_bytes == 0


# -------------------------------------------------------------------- kernels on the gpu ---
def _table(lam, state=None):
    t = np.zeros((len(lam), 8))
    t[:, 0] = lam
    if state is not None:
        t[:, 7] = state
    return t


VECTOR_CASES = [(n, K, strided) for n in (1, 63, 64, 65, 1025) for K in (1, 3, 9) for strided in (False, True)]
VECTOR_CASES.append((PCG_CAP + 1, 3, True))          # one cell past the capped grid: a second grid-stride round


@pytest.mark.gpu
@pytest.mark.parametrize('ncell, K, strided', VECTOR_CASES)
def test_vector_kernels_vs_numpy(ncell, K, strided):
    """scale -> finish -> (the existing) scalar -> direction_z against NumPy in longdouble with the table's own scalars.
    Elements: 4 eps of the magnitudes of the terms (u: a product and a quotient, 2 roundings; z: those two and the
    difference, 3; p: a product and a sum, 2). The partial sums of ``emg3d_dev_pcg_finish``, added by
    ``emg3d_dev_pcg_scalar``: ``(N + 16) eps sum |terms|``, as ``test_gauss_newton_solve``. r > 0 > g, dinv >= 0: every
    term of <r, z> is >= 0, little cancellation. Column 1 (K >= 3) is frozen, column 2 has <p,q> <= 0: their u, z, p
    keep every bit of the poison. The same calls twice: the same bits."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    rng = np.random.default_rng(ncell + 11 * K + strided)
    vpc = {1: 1, 3: 2, 9: 3}[K]
    N = vpc * ncell
    r = rng.uniform(0.5, 2.0, (K, vpc, ncell))
    g = -rng.uniform(0.5, 2.0, (K, vpc, ncell))
    act = rng.uniform(size=ncell) < 0.8 if ncell > 1 else np.array([True])
    dinv = rng.uniform(0.1, 1.0, (vpc if strided else 1, ncell)) * act
    stride = ncell if strided else 0
    poison = rng.standard_normal((3, K, vpc, ncell))
    table = _table(10 ** rng.uniform(-1, 1, K))
    table[:, 1], table[:, 2], table[:, 6] = 1.0, rng.uniform(0.5, 2.0, K), 4
    pq = rng.uniform(0.5, 2.0, K)
    if K >= 3:
        table[1, 7] = 1.0
        pq[2] = -0.25
    skipped = (1, 2) if K >= 3 else ()

    def run(first):
        ud, zd, pd = (_padded(a) for a in poison)
        rdv, gd, dd, md = _padded(r), _padded(g), _padded(dinv), _up(act.astype(np.uint8))
        td, pqd = _up(table if not first else _table(table[:, 0])), _padded(pq)
        pqp = None if first else _ptr(pqd)
        ws_len = L.emg3d_pcg_ws_len(ncell, K)
        ws = torch.full((ws_len,), float('nan'), dtype=torch.float64, device=_dev())
        _lib.check(L.emg3d_dev_pcg_scale(ncell, vpc, K, first, _ptr(ud), _ptr(rdv), _ptr(dd), stride, _ptr(td), pqp,
                                         _stream()), 'emg3d_dev_pcg_scale')
        _lib.check(L.emg3d_dev_pcg_finish(ncell, vpc, K, first, _ptr(zd), _ptr(ud), _ptr(gd), _ptr(rdv), _ptr(dd), stride,
                                          _ptr(md), _ptr(td), pqp, _ptr(ws), ws_len, _stream()), 'emg3d_dev_pcg_finish')
        _lib.check(L.emg3d_dev_pcg_scalar(ncell, K, first, 1e-3, _ptr(td), pqp, _ptr(ws), ws_len, _stream()),
                   'emg3d_dev_pcg_scalar')
        _lib.check(L.emg3d_dev_pcg_direction_z(ncell, vpc, K, first, _ptr(pd), _ptr(zd), _ptr(td), _stream()),
                   'emg3d_dev_pcg_direction_z')
        n = K * N
        return [a.cpu().numpy()[:n].reshape(K, vpc, ncell) for a in (ud, zd, pd)] + [td.cpu().numpy()]
    got = run(0)
    gu, gz, gp, gt = got
    worst = 0.0
    for k in range(K):
        if k in skipped:
            assert all(np.array_equal(a[k], b[k]) for a, b in zip((gu, gz, gp), poison))
            assert gt[k, 7] == (1 if k == 1 else 2)
            continue
        lam = LD(table[k, 0])
        want_u = dinv * r[k].astype(LD) / lam
        assert np.all(np.abs(gu[k] - want_u) <= 4 * EPS * np.abs(want_u))
        back = dinv * g[k].astype(LD) / lam
        want_z = np.where(act, gu[k] - back, 0)
        assert np.all(np.abs(gz[k] - want_z) <= 4 * EPS * (np.abs(gu[k]) + np.abs(back)))
        assert np.all(gz[k][:, ~act] == 0.0)
        rz, rr = np.sum(r[k] * gz[k].astype(LD)), np.sum(r[k].astype(LD) ** 2)
        brz, brr = (N + 16) * EPS * np.sum(np.abs(r[k] * gz[k].astype(LD))), (N + 16) * EPS * rr
        assert abs(gt[k, 2] - rz) <= brz and abs(gt[k, 5] - rr) <= brr
        worst = max(worst, float(abs(gt[k, 2] - rz) / brz) if brz else 0.0, float(abs(gt[k, 5] - rr) / brr))
        assert gt[k, 3] == table[k, 2] and gt[k, 4] == pq[k] and gt[k, 6] == 5 and gt[k, 7] == 0
        beta = LD(gt[k, 2]) / LD(gt[k, 3])
        want_p = gz[k] + beta * poison[2][k]
        assert np.all(np.abs(gp[k] - want_p) <= 4 * EPS * (np.abs(gz[k]) + np.abs(beta * poison[2][k])))
    record(f"data preconditioner vector kernels n={ncell} K={K} vpc={vpc} stride={stride}: sums max |diff| / bound = "
           f"{worst:.2e} ((N + 16) eps)")
    assert all(np.array_equal(a, b) for a, b in zip(got, run(0)))
    # the set-up: every column runs (pq is not given), p = z exactly
    fu, fz, fp, ft = run(1)
    for k in range(K):
        lam = LD(table[k, 0])
        want_u = dinv * r[k].astype(LD) / lam
        assert np.all(np.abs(fu[k] - want_u) <= 4 * EPS * np.abs(want_u))
        assert np.array_equal(fp[k], fz[k]) and ft[k, 7] == 0 and ft[k, 6] == 0 and ft[k, 1] == ft[k, 5]


def _filter(M, rho, K, Q, eig, s, d, table, y0=None):
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    qd, ed, sd, dd, td = _padded(Q), _padded(eig), _padded(s), _padded(d), _up(table)
    yd = _padded(np.full((K, M), np.nan) if y0 is None else y0)
    ws_len = L.emg3d_data_space_filter_ws_len(rho, K)
    ws = torch.full((ws_len,), float('nan'), dtype=torch.float64, device=_dev())
    _lib.check(L.emg3d_dev_data_space_filter(M, rho, K, _ptr(qd), _ptr(ed), _ptr(sd), _ptr(dd), _ptr(yd), _ptr(td), _ptr(ws),
                                             ws_len, _stream()), 'emg3d_dev_data_space_filter')
    return yd.cpu().numpy()[:K * M].reshape(K, M)


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 3, 9])
@pytest.mark.parametrize('M', [1, 12, 63, 64, 65, 257])
def test_filter_vs_numpy(M, K):
    """``y = diag(s) Q diag(phi) Q^T diag(s) d`` against longdouble for rho in {1, M // 2, M}: random orthonormal Q,
    eigenvalues over eight decades with exact zeros, s with exact zeros. Per stage a sum of M (rho) products of three
    (two) factors and phi (s) in front: ``(M + rho + 8) eps sum |terms|``; the error of stage 1 is carried through
    stage 2 with the magnitudes of its coefficients. K = 9: a second group of columns; column 1 (K >= 3) is frozen: y = 0.
    The same call twice: the same bits."""
    rng = np.random.default_rng(100 * M + K)
    full = np.linalg.qr(rng.standard_normal((M, M)))[0]
    worst = 0.0
    for rho in sorted({1, max(1, M // 2), M}):
        Q = np.ascontiguousarray(full[:, :rho])
        eig = 10 ** rng.uniform(-4, 4, rho)
        eig[rng.uniform(size=rho) < 0.2] = 0.0
        s = rng.uniform(0.5, 2.0, M)
        s[rng.uniform(size=M) < 0.2] = 0.0
        d = rng.standard_normal((K, M))
        table = _table(10 ** rng.uniform(-2, 2, K))
        if K >= 3:
            table[1, 7] = 1.0
        got = _filter(M, rho, K, Q, eig, s, d, table)
        c = (M + rho + 8) * EPS
        for k in range(K):
            if K >= 3 and k == 1:
                assert np.all(got[k] == 0.0)
                continue
            lam = LD(table[k, 0])
            phi = lam / (lam + eig.astype(LD))
            sdk = s.astype(LD) * d[k]
            t = phi * (Q.T.astype(LD) @ sdk)
            bt = c * phi * (np.abs(Q.T) @ np.abs(sdk))
            y = s * (Q.astype(LD) @ t)
            by = c * s * (np.abs(Q) @ np.abs(t)) + s * (np.abs(Q) @ bt)
            assert np.all(np.abs(got[k] - y) <= by), (M, rho, K, k)
            ok = by > 0
            worst = max(worst, float(np.max(np.abs(got[k] - y)[ok] / by[ok])) if ok.any() else 0.0)
        assert np.array_equal(got, _filter(M, rho, K, Q, eig, s, d, table))
    record(f"data_space_filter M={M} K={K}: max |diff| / bound = {worst:.2e} ((M + rho + 8) eps per stage)")


@pytest.mark.gpu
def test_bad_arguments_are_refused_and_nothing_is_launched():
    """Every refusal that the header lists: ``EMG3D_ERR_BADARG`` (too little workspace: ``EMG3D_ERR_SCRATCH``), and the
    output, filled with NaN before, is untouched."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    n, K, M, rho = 70, 2, 5, 3
    new = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float64, device=_dev())      # noqa: E731
    u, z, p, y = new(K * n), new(K * n), new(K * n), new(K * M)
    one = torch.ones(K * n, dtype=torch.float64, device=_dev())
    r, g, dinv, q = one.clone(), one.clone(), one.clone(), one.clone()
    table, pq = _up(_table([1.0, 2.0])), _up(np.ones(K))
    ws, st = new(64), _stream()
    P = _ptr
    scale = lambda **kw: L.emg3d_dev_pcg_scale(*{**dict(                                           # noqa: E731
        n=n, v=1, K=K, f=0, u=P(u), r=P(r), d=P(dinv), s=0, t=P(table), pq=P(pq), st=st), **kw}.values())
    finish = lambda **kw: L.emg3d_dev_pcg_finish(*{**dict(                                         # noqa: E731
        n=n, v=1, K=K, f=0, z=P(z), u=P(one), g=P(g), r=P(r), d=P(dinv), s=0, m=None, t=P(table), pq=P(pq), ws=P(ws), wl=64,
        st=st), **kw}.values())
    direction = lambda **kw: L.emg3d_dev_pcg_direction_z(*{**dict(                                 # noqa: E731
        n=n, v=1, K=K, f=0, p=P(p), z=P(one), t=P(table), st=st), **kw}.values())
    filt = lambda **kw: L.emg3d_dev_data_space_filter(*{**dict(                                    # noqa: E731
        M=M, rho=rho, K=K, q=P(q), e=P(one), s=P(one), d=P(r), y=P(y), t=P(table), ws=P(ws), wl=64, st=st), **kw}.values())
    bad = [scale(n=0), scale(v=0), scale(K=0), scale(K=65536), scale(u=None), scale(r=None), scale(u=P(r)), scale(d=None),
           scale(t=None), scale(s=n - 1), scale(pq=None),
           finish(n=0), finish(v=0), finish(K=0), finish(K=65536), finish(z=None), finish(u=None), finish(g=None),
           finish(r=None), finish(z=P(g)), finish(d=None), finish(t=None), finish(ws=None), finish(s=n - 1), finish(pq=None),
           direction(n=0), direction(v=0), direction(K=0), direction(K=65536), direction(p=None), direction(z=None),
           direction(z=P(p)), direction(t=None),
           filt(M=0), filt(rho=0), filt(rho=M + 1), filt(K=0), filt(q=None), filt(e=None), filt(s=None), filt(d=None),
           filt(y=None), filt(y=P(r)), filt(t=None)]
    assert all(status == BADARG for status in bad), bad
    assert finish(wl=1) == SCRATCH and filt(wl=rho * K - 1) == SCRATCH and filt(ws=None) == SCRATCH
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (u, z, p, y))
    assert scale(pq=None, f=1) == 0 and finish(pq=None, f=1) == 0       # the set-up takes no <p,q>
    torch.cuda.synchronize()


# ------------------------------------------------------- the preconditioner on the gpu ---
IRLS = dict(norms=(1.0, 1.0, 1.0, 1.0), irls_eps=(1e-2, 1e-3))


@functools.lru_cache(maxsize=None)
def _parts(name, masked=False, irls=False):
    """Per case, once: the instance of ``test_gauss_newton_solve._dense`` (after ``forward()``), dense H from
    ``hessian_vec_block`` on the identity as that function forms it, dense R from ``regulariser_vec_block`` on the
    identity (with ``irls``: cell weights and norms (1, 1, 1, 1) at a random linearisation point), the active entries,
    the keyword arguments of R, and the sensitivity J^ (M, N) from ``jtvec_block`` on the unit data."""
    import torch
    grid, rec, active, act, lams, b, dense = _dense(name, masked)
    n, ncell = gradient._NCOMP[rec.model.case], grid.n_cells
    N = n * ncell
    eye = torch.eye(N, dtype=torch.float64, device=_dev()).view(N, n, ncell)
    H = np.concatenate([_columns(rec.hessian_vec_block(eye[c:c + KC].contiguous(), columns_per_pass=KC))
                        for c in range(0, N, KC)]).T
    reg = dict(REG, active=active)
    if irls:
        rng = np.random.default_rng(17)
        reg.update(IRLS, cell_weights=rng.uniform(0.5, 2.0, grid.shape_cells),
                   linearise_at=rng.standard_normal(((n,) if n > 1 else ()) + tuple(grid.shape_cells)) * 0.05)
    R = _columns(rec.regulariser_vec_block(eye, **reg)).T
    M = 2 * len(rec.pairs) * len(RECS)
    J = _columns(rec.jtvec_block([rec.unstack_data(e) for e in np.eye(M)], on_device=True))
    return grid, rec, reg, act, H, R, J


def _weights(rec, rng):
    """Data weights over two decades with one exact zero."""
    w = {pair: 10 ** rng.uniform(-1, 1, len(RECS)) for pair in rec.pairs}
    w[rec.pairs[-1]][1] = 0.0
    return w


def _bound_factor(grid, N, M):
    """The ``c`` of ``c cond_2 eps``: the preconditioner and the dense matrix it is compared with are both built from
    sums over at most ``n_edges`` products (the field products of a pass), ``N`` (the data-space matrix, one row of a dense
    product) and ``M`` terms (the data-space sums), each product of up to four factors: 4 (n_edges + N + M) roundings bound
    the relative perturbation of either matrix, and a relative perturbation delta of a matrix moves the solution of a
    system with it by at most ``cond_2 delta`` to first order."""
    return 4 * (grid.n_edges + N + M)


@pytest.mark.gpu
@pytest.mark.parametrize('name, masked, irls', [('isotropic', False, False), ('isotropic', True, False),
                                                ('triaxial', False, False), ('isotropic', False, True)],
                         ids=['isotropic', 'masked', 'triaxial', 'weighted-l1'])
def test_preconditioner_vs_dense_inverse(name, masked, irls):
    """``M_k`` through the helper, applied to a random block, against NumPy's dense ``(lambda_k diag R + H)^-1`` on the
    active cells with the dense ``H`` of ``hessian_vec_block`` on the identity (unit weights, all M eigenpairs); its
    symmetry; and, with ``data_rank = 8`` of M = 12 and weights of which one is zero, against the dense inverse of the
    truncated operator ``lambda_k diag R + J^T diag(s) Q_8 Q_8^T diag(s) J^`` built from the same Q and the dense
    sensitivity. Bounds: ``_bound_factor``."""
    grid, rec, reg, act, H, R, J = _parts(name, masked, irls)
    N, M = H.shape[0], J.shape[0]
    rng = np.random.default_rng(23)
    lams = np.trace(H[act][:, act]) / np.trace(R) * np.array([1e-2, 1.0, 1e2])
    rdiag = np.diagonal(R)
    dinv_want = np.where(act, np.where(rdiag > 0, 1.0 / np.where(rdiag > 0, rdiag, 1.0), 1.0), 0.0)
    blocks = rng.standard_normal((2, 3, N)) * act
    c = _bound_factor(grid, N, M)
    for rank, w in ((None, None), (8, _weights(rec, rng))):
        pre, apply = rec._data_preconditioner(lams, weights=w, data_rank=rank, **reg)
        rho = M if rank is None else rank
        s = np.ones(M) if w is None else rec.stack_data({p: np.sqrt(v) * (1 + 1j) for p, v in w.items()})
        assert pre['rank'] == rho and pre['n_data'] == M and tuple(pre['q'].shape) == (M, rho)
        assert np.array_equal(pre['s_host'], s)
        dinv = pre['dinv'].cpu().numpy().ravel()
        # (the diagonal kernel and the operator on unit vectors add the same coefficients in another order: 32 eps)
        assert np.all(np.abs(np.tile(dinv, N // dinv.size) - dinv_want) <= 64 * EPS * dinv_want)
        assert np.all(np.diff(pre['eigenvalues_host']) <= 0) and np.all(pre['eigenvalues_host'] >= 0)
        T = J.T @ (s[:, None] * pre['q_host'])                      # N x rho: H_rho = T T^T
        za, zb = (_columns(apply(_up(blk.reshape(3, -1, grid.n_cells)))) for blk in blocks)
        worst = wsym = 0.0
        for k, lam in enumerate(lams):
            A = (lam * np.diag(rdiag) + (H if rank is None else T @ T.T))[act][:, act]
            ev = np.linalg.eigvalsh((A + A.T) / 2)
            cond = ev[-1] / ev[0]
            for got, blk in ((za, blocks[0]), (zb, blocks[1])):
                want = np.linalg.solve(A, blk[k][act])
                assert np.all(got[k][~act] == 0.0)
                err = np.linalg.norm(got[k][act] - want) / np.linalg.norm(want)
                assert err <= c * cond * EPS, (name, rank, k, err, cond)
                worst = max(worst, err / (c * cond * EPS))
            a, b = blocks[0][k], blocks[1][k]
            sym = abs(a @ zb[k] - za[k] @ b)
            bsym = c * cond * EPS * (np.linalg.norm(a) * np.linalg.norm(zb[k]) + np.linalg.norm(za[k]) * np.linalg.norm(b))
            assert sym <= bsym
            wsym = max(wsym, sym / bsym)
        record(f"data preconditioner {name} masked={masked} irls={irls} rank {rho} of {M}: max |z - dense| / (c cond eps "
               f"|z|) = {worst:.2e}, symmetry / bound = {wsym:.2e}, c = {c}")


# ------------------------------------------------------------------ the solve on the gpu ---
def _pcg_dense(A, b, Minv, tol, maxit=5000):
    """Textbook PCG with a dense preconditioner ``Minv``: the iterations to ``|r| <= tol |b|``."""
    x, r = np.zeros_like(b), b.copy()
    z = Minv @ r
    p, rz = z.copy(), r @ z
    for it in range(1, maxit + 1):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        if np.linalg.norm(r) <= tol * np.linalg.norm(b):
            return it
        z = Minv @ r
        rz, old = r @ z, rz
        p = z + rz / old * p
    raise AssertionError("the dense model's own PCG did not converge")


DIAGONAL = dict(smallness=2e-3, smoothness=(0.0, 0.0, 0.0))


def _diagonal_case():
    """Smallness only: R = smallness diag(V) is diagonal. Weights with one zero, three dampings over four decades
    around trace(H) / trace(R), random right-hand sides; dense H_w = J^T W J and the diagonal of R."""
    grid, rec, reg, act, H, R, J = _parts('isotropic')
    rng = np.random.default_rng(31)
    w = _weights(rec, rng)
    s = rec.stack_data({p: np.sqrt(v) * (1 + 1j) for p, v in w.items()})
    Hw = J.T @ ((s ** 2)[:, None] * J)
    rdiag = DIAGONAL['smallness'] * grid.cell_volumes.ravel(order='F')
    lams = np.trace(Hw) / rdiag.sum() * np.array([1e-2, 1.0, 1e2])
    b = rng.standard_normal((3, H.shape[0]))
    return grid, rec, w, s, J, Hw, rdiag, lams, b


@pytest.mark.gpu
def test_diagonal_regulariser_converges_at_once():
    """With a diagonal R the preconditioner is the exact inverse: PCG converges in 1 iteration in exact arithmetic, a
    second is the allowance for rounding. The dense model (NumPy, same H, same M) confirms it before the GPU is asked.
    Jacobi's count on the same call is recorded."""
    grid, rec, w, s, J, Hw, rdiag, lams, b = _diagonal_case()
    for lam, bk in zip(lams, b):
        A = lam * np.diag(rdiag) + Hw
        assert _pcg_dense(A, bk, np.linalg.inv(A), 1e-8) <= 2
    rhs = _to_model(rec, grid, b)
    x, info = rec.gauss_newton_solve(rhs, lams, weights=w, tol=1e-8, maxit=20, precondition='data', **DIAGONAL)
    jac = rec.gauss_newton_solve(rhs, lams, weights=w, tol=1e-8, maxit=100, **DIAGONAL)[1]
    record(f"gauss_newton_solve diagonal R: iterations data {info['iterations'].tolist()}, Jacobi "
           f"{jac['iterations'].tolist()} (states {jac['state'].tolist()}, maxit 100)")
    assert np.all(info['state'] == 1) and np.all(info['iterations'] <= 2), info
    assert info['data_rank'] == 12 and info['preconditioner_passes'] == info['hessian_passes'] + 1
    x = _from_model(x)
    for k, (lam, bk) in enumerate(zip(lams, b)):
        A = lam * np.diag(rdiag) + Hw
        assert np.linalg.norm(bk - A @ x[k]) <= 2e-8 * np.linalg.norm(bk)


@pytest.mark.gpu
def test_truncated_rank_needs_one_iteration_per_eigenvalue_left_out():
    """``data_rank = rho < rank B``: M is the inverse of ``A - T_rest T_rest^T``, so ``M A`` is the identity plus a term of
    rank ``rank(B) - rho``: at most that many + 1 distinct eigenvalues, PCG ends within as many iterations in exact
    arithmetic; one more is the allowance for rounding. rank(B) and the dense model's own count come from NumPy."""
    grid, rec, w, s, J, Hw, rdiag, lams, b = _diagonal_case()
    rho = 7
    pre, _ = rec._data_preconditioner(lams, weights=w, data_rank=rho, **DIAGONAL)
    eig = pre['eigenvalues_host']
    rank_b = int(np.sum(eig > len(eig) * EPS * eig[0]))
    assert rho < rank_b <= 10                        # one datum has weight 0: its Re and Im rows of B vanish
    T = J.T @ (s[:, None] * pre['q_host'])
    for lam, bk in zip(lams, b):
        A = lam * np.diag(rdiag) + Hw
        model = _pcg_dense(A, bk, np.linalg.inv(lam * np.diag(rdiag) + T @ T.T), 1e-8)
        assert model <= rank_b - rho + 2, (model, rank_b)
    x, info = rec.gauss_newton_solve(_to_model(rec, grid, b), lams, weights=w, tol=1e-8, maxit=20, precondition='data',
                                     data_rank=rho, **DIAGONAL)
    record(f"gauss_newton_solve diagonal R, rank {rho} of {rank_b}: iterations {info['iterations'].tolist()} "
           f"(bound {rank_b - rho + 2})")
    assert np.all(info['state'] == 1) and np.all(info['iterations'] <= rank_b - rho + 2) and info['data_rank'] == rho


@functools.lru_cache(maxsize=None)
def _smooth(name='isotropic'):
    """The smooth R of ``test_gauss_newton_solve`` with its dense systems; per damping the iterations of the dense model
    with the dense Woodbury preconditioner, and those without a preconditioner."""
    grid, rec, active, act, lams, b, dense = _dense(name)
    _, _, reg, _, H, R, J = _parts(name)
    its, plain = [], []
    for lam, bk, (A, xs, cond, jac) in zip(lams, b, dense):
        Minv = np.linalg.inv(lam * np.diag(np.diagonal(R)) + H)
        its.append(_pcg_dense(A, bk, Minv, TOL))
        plain.append(_pcg_numpy(A, bk, np.ones(len(A)), TOL, 20000))
    return grid, rec, act, lams, b, dense, its, plain


@pytest.mark.gpu
def test_solve_vs_dense():
    """Smooth R, three dampings, tol 1e-10: the checks of ``_check_solution`` within twice the dense model's count + 10.
    The counts are recorded beside Jacobi's and the unpreconditioned ones of the dense models; none is asserted against
    another."""
    grid, rec, act, lams, b, dense, its, plain = _smooth()
    before = dict(rec.n_solves)
    x, info = rec.gauss_newton_solve(_to_model(rec, grid, b), lams, tol=TOL, maxit=2 * max(its) + 10, precondition='data',
                                     columns_per_pass=KC, **REG)
    record(f"gauss_newton_solve smooth R: iterations data {info['iterations'].tolist()} (dense model {its}), dense "
           f"Jacobi {[d[3] for d in dense]}, dense unpreconditioned {plain}")
    _check_solution("precondition='data'", dense, _from_model(x), info, act, b)
    assert info['preconditioner_passes'] == info['hessian_passes'] + 1 and info['data_rank'] == 12
    assert rec.n_solves == before


@pytest.mark.gpu
def test_check_every_changes_no_bit_and_host_kept_fields_give_the_same_bits():
    grid, rec, act, lams, b, dense, its, plain = _smooth()
    rhs = _to_model(rec, grid, b[:2])
    lam = np.array([1e4 * lams[1], lams[1]])
    args = dict(tol=1e-8, maxit=2 * max(its) + 10, precondition='data', **REG)
    (x1, i1), (x3, i3) = (rec.gauss_newton_solve(rhs, lam, check_every=ce, **args) for ce in (1, 3))
    assert np.all(i1['state'] == 1) and np.array_equal(x1, x3) and np.array_equal(i1['iterations'], i3['iterations'])
    assert np.array_equal(i1['relative_residual'], i3['relative_residual'])
    record(f"gauss_newton_solve data, freezing: iterations {i1['iterations'].tolist()}, passes {i1['hessian_passes']} / "
           f"{i3['hessian_passes']} with check_every 1 / 3")
    grid2, other = _survey('isotropic', keep='host')
    xh, ih = other.gauss_newton_solve(rhs, lam, check_every=1, **args)
    assert np.array_equal(xh, x1) and np.array_equal(ih['iterations'], i1['iterations'])


@pytest.mark.gpu
def test_single_precision_fields():
    """``field_dtype='single'`` against ``'double'``: both solve their own system to ``tol``, which differ by the
    rounding of the kept fields, relative 2^-24 per value -- the 1e-7 class of DESIGN.md 4.15, for which
    ``test_gauss_newton_solve.test_storage_variants`` allows 1e-6 between the storage types: ``2 cond tol + 1e-6``."""
    grid, rec, act, lams, b, dense, its, plain = _smooth()
    rhs = _to_model(rec, grid, b)
    args = dict(tol=TOL, maxit=2 * max(its) + 10, precondition='data', **REG)
    want = _from_model(rec.gauss_newton_solve(rhs, lams, **args)[0])
    grid2, other = _survey('isotropic', field_dtype='single')
    x, info = other.gauss_newton_solve(rhs, lams, **args)
    x = _from_model(x)
    assert np.all(info['state'] == 1)
    for k, (A, xs, cond, jac) in enumerate(dense):
        rel = np.linalg.norm(x[k] - want[k]) / np.linalg.norm(xs)
        record(f"gauss_newton_solve data, single: column {k} |x - x_double| / |x*| = {rel:.2e} "
               f"(bound {2 * cond * TOL + 1e-6:.2e})")
        assert rel <= 2 * cond * TOL + 1e-6


# the C calls of an iteration of the routes that existed before, with the number of their arguments
OLD_CALLS = {'emg3d_dev_pcg_update': 16, 'emg3d_dev_pcg_scalar': 9, 'emg3d_dev_pcg_direction': 11,
             'emg3d_dev_model_regulariser': 21, 'emg3d_dev_model_regulariser_diagonal': 13, 'emg3d_dev_hessian_diagonal': 19,
             'emg3d_dev_edge_weights': 11, 'emg3d_dev_sensitivity_dots_block': 17, 'emg3d_dev_sensitivity_combine_block': 13,
             'emg3d_dev_edges_to_cells': 14, 'emg3d_pcg_table_len': 1, 'emg3d_pcg_ws_len': 2,
             'emg3d_model_regulariser_ws_len': 5, 'emg3d_sensitivity_dots_block_ws_len': 4}


@pytest.mark.gpu
def test_the_other_routes_reach_no_new_entry_point(monkeypatch):
    """A recorder around the library: ``precondition`` True and False call the entry points they called before, with
    argument lists of the same lengths, Jacobi with both diagonals and without them; ``'data'`` calls the new ones."""
    grid, rec, act, lams, b, dense, its, plain = _smooth()
    real = _lib.lib()
    calls = []

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def wrapped(*args):
                calls.append((name, args))
                return fn(*args)
            return wrapped
    monkeypatch.setattr(_lib, 'lib', lambda: Recorder())
    rhs = _to_model(rec, grid, b)
    for precondition in (True, False):
        calls.clear()
        rec.gauss_newton_solve(rhs, lams, tol=1e-3, maxit=3, precondition=precondition, **REG)
        names = {name for name, _ in calls}
        assert not names & set(SYMBOLS), names & set(SYMBOLS)
        assert {n for n in names if n.startswith('emg3d_dev_')} <= set(OLD_CALLS), names - set(OLD_CALLS)
        assert {'emg3d_dev_pcg_update', 'emg3d_dev_pcg_scalar', 'emg3d_dev_pcg_direction'} <= names
        assert all(len(args) == OLD_CALLS[name] for name, args in calls if name in OLD_CALLS)
        for name, args in calls:
            if name == 'emg3d_dev_pcg_update':
                assert (args[8] is not None and args[9] is not None) == precondition
            if name == 'emg3d_dev_pcg_direction':
                assert (args[6] is not None and args[7] is not None) == precondition
        assert ('emg3d_dev_hessian_diagonal' in names) == precondition
    calls.clear()
    rec.gauss_newton_solve(rhs, lams, tol=1e-3, maxit=3, precondition='data', **REG)
    names = {name for name, _ in calls}
    assert {'emg3d_dev_pcg_scale', 'emg3d_dev_data_space_filter', 'emg3d_dev_pcg_finish',
            'emg3d_dev_pcg_direction_z'} <= names and 'emg3d_dev_pcg_direction' not in names
