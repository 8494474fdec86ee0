"""The capped grids and the second-stage sums past their first pass.

Most reductions of ``csrc/reciprocal.h``, ``csrc/block.h`` and ``csrc/regularise.h`` end in ONE workgroup of 256 threads
that adds the first stage's partial sums with ``for (i = tid; i < count; i += 256)``; the PCG kernels and
``k_any_real_part`` (behind ``emg3d_dev_eta_is_imaginary``) run on a grid capped at 1024 workgroups of 256 threads with a
grid-stride loop. The tests of the kernels' own files stop short of the sizes at which these loops go round a second
time; the sizes here are the smallest that reach the second pass, and the third where a case says so:

    k_sensitivity_dots_final after k_sensitivity_dots         n > 256 * 8192 (one partial per chunk of 8192)
    the same after k_sensitivity_dots_block                   n > 256 * 4096 (one partial per chunk of 4096)
    k_regulariser_finish                                      more than 256 waves (one partial per wave)
    k_pcg_scalar                                              n_cells > 65 536 (one partial per workgroup)
    k_pcg_update, k_pcg_direction                             n_cells > 262 144 (1024 workgroups x 256)
    k_any_real_part                                           n_cells > 262 144 (the same grid)

The callers and checkers are those of ``test_reciprocal``, ``test_block_products`` and ``test_gauss_newton_solve``: every
workspace and output starts as NaN, every buffer is followed by NaN, every case runs twice and must give the same bits.
The bounds are the ones those files derive -- ``(N + 16) eps sum |terms|`` for a sum, ``4 eps`` of the magnitudes for an
element of the PCG kernels, ``16 eps sum |terms|`` for an output of the regulariser -- against NumPy in ``longdouble``.

A dropped partial must not be able to hide behind a bound that grows with N. The inputs have little cancellation
(weights, and the real and imaginary parts of field values, in [0.5, 1.5]), and every sum test first computes, from the
reference alone, the partial that each first-stage unit contributes (a chunk, a wave, the cells of a workgroup) and
asserts ``min |partial| >= 100 bound`` of that entry: a condition on the inputs, checked before the kernel's result is
looked at. A unit without any term (a wave of the regulariser outside the grid, or on inactive cells only with beta = 0)
contributes an exact 0, which cannot be dropped wrongly; it is left out of the minimum, and every pass of the final loop
is asserted to hold at least one unit that is not.

Figures that the tests observe are printed and, with ``EMG3D_AMD_PARITY_FILE`` set, appended to that file
(``profiles/reduction_passes_parity.txt`` is such a run).
"""
import ctypes
import itertools

import numpy as np
import pytest

from emg3d_amd import _lib
from test_block_products import _dots_block, _dots_single, _inputs
from test_gauss_newton_solve import ALPHAS, _flat, _pcg, _regulariser, _z_numpy, regulariser_numpy
from test_reciprocal import _dots, _stack, _up
from test_sensitivity import EPS, record

LD = np.longdouble
DOT_CHUNK, DB_CHUNK = 8192, 4096          # elements per partial of k_sensitivity_dots and of k_sensitivity_dots_block
FINAL = 256                               # threads of every second stage: partial i is added by thread i % 256
PCG_GRID = 1024                           # workgroups (of 256 threads) at which the PCG grid and k_any_real_part's is capped
ROUND = PCG_GRID * 256                    # elements of one round of a grid-stride loop
MARGIN = 100.0                            # min |partial| >= MARGIN * bound: the condition on the inputs


def _fill(rng, a, n):
    """Values with little cancellation into ``a[:, :n]``: real and imaginary parts in [0.5, 1.5]. What lies behind n
    (NaN) stays."""
    v = rng.uniform(0.5, 1.5, (len(a), n))
    if a.dtype.kind == 'c':
        v = v + 1j * rng.uniform(0.5, 1.5, (len(a), n))
    a[:, :n] = v


def _passes(count):
    return -(-count // FINAL)


# --------------------------------------------------------------------------------- dots ---
def _pair_terms(e, x):
    """``e[k] x[k]`` in longdouble as (real part, imaginary part or None)."""
    if np.iscomplexobj(e):
        a, b, c, d = (v.astype(LD) for v in (e.real, e.imag, x.real, x.imag))
        return a * c - b * d, a * d + b * c
    return e.astype(LD) * x.astype(LD), None


def _dots_reference(W, E, X, scale, chunk):
    """For ``out[v, s, r] = scale sum_k W[v, k] E[s, k] X[r, k]``, one (s, r) pair at a time in longdouble: the sums, the
    bound ``(n + 16) eps |scale| sum |w| |e| |x|`` and, per entry, the smallest ``|scale partial|`` over the chunks."""
    nv, ns, nr, n = len(W), len(E), len(X), W.shape[1]
    is_complex = np.iscomplexobj(E)
    starts = np.arange(0, n, chunk)
    want = np.zeros((nv, ns, nr), dtype=np.clongdouble if is_complex else LD)
    least, mag = np.zeros((nv, ns, nr)), np.zeros((nv, ns, nr))
    Wl = [w.astype(LD) for w in W]
    for s, r in itertools.product(range(ns), range(nr)):
        re, im = _pair_terms(E[s], X[r])
        size = np.abs(E[s]) * np.abs(X[r])
        for v in range(nv):
            part = np.add.reduceat(Wl[v] * re, starts)
            if is_complex:
                part = part + 1j * np.add.reduceat(Wl[v] * im, starts)
            part = (np.clongdouble(scale) if is_complex else LD(scale)) * part
            want[v, s, r] = part.sum()
            least[v, s, r] = float(np.min(np.abs(part)))
            mag[v, s, r] = np.abs(W[v]) @ size
    return want, (n + 16) * EPS * abs(scale) * mag, least


def _scale(is_complex):
    return 0.3 - 1.7j if is_complex else 0.7


def _dots_inputs(n, ns, nr, is_complex):
    rng = np.random.default_rng(n + 10 * ns + nr + is_complex)
    (E, es), (X, xs) = _stack(rng, ns, n, is_complex), _stack(rng, nr, n, is_complex)
    _fill(rng, E, n)
    _fill(rng, X, n)
    return E, es, X, xs, rng.uniform(0.5, 1.5, n)


def _positive_inputs(seed, n, ns, nr, nv, is_complex, storage):
    """``test_block_products._inputs`` (strides, NaN padding, alignment) with values of little cancellation."""
    d = _inputs(seed, n, ns, nr, nv, is_complex, storage)
    rng = np.random.default_rng(seed + 1)
    for key in 'EXW':
        _fill(rng, d[key], n)
    d['Ew'], d['Xw'] = (d[key][:, :n].astype(d['wide']) for key in 'EX')
    return d


def _check_sums(tag, got, want, bound, least, nchunk):
    """The condition on the inputs has been asserted by the caller; here: no NaN, every entry within its bound."""
    assert not np.any(np.isnan(got))
    ratio = np.abs(got - want) / bound
    record(f"{tag}: {nchunk} partials, passes of the final loop: {_passes(nchunk)}; min |partial| / bound = "
           f"{float(np.min(least / bound)):.2e} (needs {MARGIN:.0f}); max |diff| / bound = {float(np.max(ratio)):.2e} (bound (n + 16) "
           f"eps)")
    assert np.all(ratio <= 1)


DOTS = [(256 * DOT_CHUNK, True), (256 * DOT_CHUNK, False),                # 256 partials: the last size with one pass
        (256 * DOT_CHUNK + 1, True), (256 * DOT_CHUNK + 1, False),        # 257: the last from a chunk of ONE element
        (512 * DOT_CHUNK + DOT_CHUNK // 2 + 3, False)]                    # 513: thread 0 adds three


@pytest.mark.gpu
@pytest.mark.parametrize('n, is_complex', DOTS)
def test_dots_final_past_one_pass(n, is_complex):
    """``emg3d_dev_sensitivity_dots`` with (ns, nr) = (2, 3), a ragged 4 x 4 tile: per entry ``|got - want| <= (n + 16)
    eps |scale| sum_k |w_k| |e_s[k]| |x_r[k]|`` against longdouble; before that, every chunk's partial is at least 100
    bounds (the lone element of the 257th chunk included). Twice: the same bits."""
    ns, nr = 2, 3
    E, es, X, xs, w = _dots_inputs(n, ns, nr, is_complex)
    scale = _scale(is_complex)
    nchunk = -(-n // DOT_CHUNK)
    assert _lib.lib().emg3d_sensitivity_dots_ws_len(ns, nr, n) == 2 * ns * nr * nchunk
    want, bound, least = _dots_reference(w[None], E[:, :n], X[:, :n], scale, DOT_CHUNK)
    assert np.all(least >= MARGIN * bound)                       # the inputs: no partial can hide in the bound
    Ed, Xd, wd = _up(E), _up(X), _up(w)
    got = _dots(Ed, es, Xd, xs, n, wd, scale, is_complex)
    assert got.dtype == E.dtype
    _check_sums(f"dots n={n} ns={ns} nr={nr} complex={is_complex}", got, want[0], bound[0], least[0], nchunk)
    assert np.array_equal(got, _dots(Ed, es, Xd, xs, n, wd, scale, is_complex))


@pytest.mark.gpu
def test_dots_sp_final_past_one_pass():
    """``emg3d_dev_sensitivity_dots_sp`` on complex64 stacks whose rows lie on 16 bytes: the instantiation with 16-byte
    loads feeds 257 partials to the final kernel. Reference on the widened values."""
    n, ns, nr = 256 * DOT_CHUNK + 1, 2, 3
    d = _positive_inputs(n + 7, n, ns, nr, 1, True, 'sp-aligned')
    assert d['E'].dtype == np.complex64 and d['es'] * 8 % 16 == 0 and d['xs'] * 8 % 16 == 0
    scale = _scale(True)
    nchunk = -(-n // DOT_CHUNK)
    want, bound, least = _dots_reference(d['W'][:, :n], d['Ew'], d['Xw'], scale, DOT_CHUNK)
    assert np.all(least >= MARGIN * bound)
    Ed, Xd, Wd = _up(d['E']), _up(d['X']), _up(d['W'])
    assert Ed.data_ptr() % 16 == 0 and Xd.data_ptr() % 16 == 0 and Wd.data_ptr() % 16 == 0
    got = _dots_single(d, Ed, Xd, Wd, n, 0, scale, True)
    _check_sums(f"dots_sp n={n} ns={ns} nr={nr} complex=True sp-aligned", got, want[0], bound[0], least[0], nchunk)
    assert np.array_equal(got, _dots_single(d, Ed, Xd, Wd, n, 0, scale, True))


# (ns, nr, nv): (3, 5, 5) is 2 x 2 x 2 = 8 tiles, ONE group of 8 waves; (1, 9, 9) is 1 x 3 x 3 = 9 tiles, two groups, the
# second with one live wave and seven that return at once -- 2 x 257 = 514 workgroups, decoded by blockIdx.x / 2 and % 2;
# 'sp-aligned' (float32, four values per 16-byte load) is 1 x 1 x 2 tiles
BLOCKS = [(256 * DB_CHUNK, 3, 5, 5, True, 'fp64'), (256 * DB_CHUNK + 1, 3, 5, 5, True, 'fp64'),
          (256 * DB_CHUNK, 1, 9, 9, False, 'fp64'), (256 * DB_CHUNK + 1, 1, 9, 9, False, 'fp64'),
          (256 * DB_CHUNK + 1, 2, 3, 5, False, 'sp-aligned')]


@pytest.mark.gpu
@pytest.mark.parametrize('n, ns, nr, nv, is_complex, storage', BLOCKS)
def test_dots_block_final_past_one_pass(n, ns, nr, nv, is_complex, storage):
    """``emg3d_dev_sensitivity_dots_block`` at 256 and 257 partials per entry against longdouble and, column by column,
    against ``emg3d_dev_sensitivity_dots`` -- which at this n has 129 partials and ONE pass of the final kernel: an
    independent route --, both within ``(n + 16) eps |scale| sum_k |w_v[k]| |e_s[k]| |x_r[k]|``. Twice: the same bits."""
    d = _positive_inputs(n + 10 * ns + nr + 100 * nv + is_complex, n, ns, nr, nv, is_complex, storage)
    scale = _scale(is_complex)
    nchunk = -(-n // DB_CHUNK)
    assert _lib.lib().emg3d_sensitivity_dots_block_ws_len(ns, nr, nv, n) == 2 * nv * ns * nr * nchunk
    assert -(-n // DOT_CHUNK) <= FINAL                           # (the route of the comparison: one pass)
    want, bound, least = _dots_reference(d['W'][:, :n], d['Ew'], d['Xw'], scale, DB_CHUNK)
    assert np.all(least >= MARGIN * bound)
    Ed, Xd, Wd = _up(d['E']), _up(d['X']), _up(d['W'])
    got = _dots_block(d, Ed, Xd, Wd, n, nv, scale, is_complex)
    assert got.dtype == d['wide']
    _check_sums(f"dots_block n={n} ns={ns} nr={nr} nv={nv} complex={is_complex} {storage}", got, want, bound, least, nchunk)
    single = np.stack([_dots_single(d, Ed, Xd, Wd, n, v, scale, is_complex) for v in range(nv)])
    worst = float(np.max(np.abs(got - single) / bound))
    record(f"dots_block n={n} ns={ns} nr={nr} nv={nv} complex={is_complex} {storage}: max |diff| / bound = {worst:.2e} vs dots "
           f"per column ({-(-n // DOT_CHUNK)} partials, one pass)")
    assert np.all(np.abs(got - single) <= bound)
    assert np.array_equal(got, _dots_block(d, Ed, Xd, Wd, n, nv, scale, is_complex))


# -------------------------------------------------------------------------- regulariser ---
SMALLNESS = (20.0, 1.0, 0.5, 2.0)         # with widths of about one, alpha_s V is ten times what the faces add: p q > 0 per cell
REG_SHAPES = [(1, 1, 65),                 # 260 partials, three of four waves hold no cell
              (3, 2, 70),                 # 280
              (65, 9, 11),                # 264: 2 x 3 workgroups in x and y
              (130, 5, 52)]               # 1248: five passes; 3 x 2 workgroups in 52 planes
REG_VECTORS = [(3, 1), (9, 3)]            # (nvec, vec_per_col)


def _mild_widths(n, first, rng):
    """n non-uniform widths within a factor of 5 / 3 of each other, and of about one: no cell may dwarf another in a sum,
    nor R p the beta q0 of an inactive cell."""
    return first * rng.uniform(0.75, 1.25, n)


def _wave_sums(t, count):
    """t (nx, ny, nz): per cell the longdouble terms of a column; count: per cell how many of them exist. Returns the
    partial of every wave of ``k_model_regulariser`` -- 64 cells along x at one (iy, iz), wave = 4 x (linear workgroup
    index, x fastest) + iy % 4 -- and which waves hold a term at all."""
    nx, ny, nz = t.shape
    gx, gy = -(-nx // 64), -(-ny // 4)

    def fold(a):
        full = np.zeros((gx * 64, gy * 4, nz), dtype=a.dtype)
        full[:nx, :ny] = a
        return full.reshape(gx, 64, gy, 4, nz).sum(axis=1).transpose(3, 1, 0, 2).ravel()          # (bz, by, bx, ty)
    return fold(t), fold(count) > 0


@pytest.mark.gpu
@pytest.mark.parametrize('shape', REG_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_regulariser_finish_past_one_pass(shape):
    """``emg3d_dev_model_regulariser`` with ``pq`` where ``k_regulariser_finish`` adds more than 256 partials per
    column. ``|<p,q> - want| <= (N + 16) eps sum |p| |q|``, N the elements of a column, against the longdouble sum over
    the kernel's own q (as ``test_regulariser_vs_numpy``), and every q within ``16 eps (|beta q0| + |lam| sum |terms
    of R p|)``. Before that, from the reference alone: every wave that holds a term contributes at least 100 bounds, and
    every pass of the final loop has such a wave. Vector layouts (3, 1) and (9, 3), no mask and a random one, the
    coefficient set ``ALPHAS[-1]`` and a smallness-dominated one, beta 0 (no lambda) and 1 (a lambda per column). Each
    case twice: the same bits."""
    nx, ny, nz = shape
    rng = np.random.default_rng(1000 * nx + 10 * ny + nz + 5)
    h = [_mild_widths(nx, 1.0, rng), _mild_widths(ny, 1.4, rng), _mild_widths(nz, 0.6, rng)]
    ncell = nx * ny * nz
    nparts = -(-nx // 64) * -(-ny // 4) * nz * 4
    random_mask = rng.uniform(size=shape) < 0.7
    random_mask[-1, -1, -1] = True                               # (1, 1, 65): the one cell of the second pass
    worst_q = worst_pq = 0.0
    least = np.inf
    for (nvec, vpc), mask, alphas, beta in itertools.product(REG_VECTORS, (None, random_mask), (ALPHAS[-1], SMALLNESS),
                                                             (0.0, 1.0)):
        case = (nvec, vpc, mask is not None, alphas, beta)
        ncol = nvec // vpc
        assert _lib.lib().emg3d_model_regulariser_ws_len(nx, ny, nz, nvec, vpc) == ncol * nparts
        p = rng.uniform(0.5, 1.5, (nvec,) + shape)
        q0 = rng.uniform(0.5, 1.5, (nvec, ncell)) if beta else None
        lam = 10 ** rng.uniform(-1, 1, ncol) if beta else None
        rp, mag = regulariser_numpy(h, alphas, mask, p)
        lcol = np.repeat(np.ones(ncol) if lam is None else lam, vpc).astype(LD)[:, None]
        want = lcol * _flat(rp) + (beta * q0.astype(LD) if beta else 0)
        bound = 16 * EPS * (lcol * _flat(mag) + (np.abs(beta * q0) if beta else 0))
        # the inputs: the partial of every wave, from the reference alone
        pf = _flat(p).astype(LD)
        terms = (pf * want).reshape(ncol, vpc, nz, ny, nx).transpose(0, 1, 4, 3, 2)          # cells x fastest
        exists = np.ones(shape) if (mask is None or beta) else mask.astype(float)
        for col in range(ncol):
            part, live = _wave_sums(terms[col].sum(axis=0), exists)
            ref_bound = (vpc * ncell + 16) * EPS * float(np.sum(np.abs(terms[col])))
            assert len(part) == nparts and np.all(part[~live] == 0)
            assert all(np.any(live[i:i + FINAL]) for i in range(0, nparts, FINAL)), case      # every pass adds something
            assert np.min(np.abs(part[live])) >= MARGIN * ref_bound, case
            least = min(least, float(np.min(np.abs(part[live])) / ref_bound))
        got, pq = _regulariser(h, alphas, mask, p, q0, beta, lam, vpc)
        assert not np.any(np.isnan(got)) and not np.any(np.isnan(pq))
        err = np.abs(got - want)
        assert np.all(err <= bound), case
        if mask is not None and not beta:
            assert np.all(got[:, ~mask.ravel(order='F')] == 0.0)
        worst_q = max(worst_q, float(np.max(err[bound > 0] / bound[bound > 0])))
        want_pq = np.sum((pf * got.astype(LD)).reshape(ncol, -1), axis=1)
        bound_pq = (vpc * ncell + 16) * EPS * np.sum(np.abs(pf * got).reshape(ncol, -1), axis=1)
        assert np.all(np.abs(pq - want_pq) <= bound_pq), case
        worst_pq = max(worst_pq, float(np.max(np.abs(pq - want_pq) / bound_pq)))
        again, pq2 = _regulariser(h, alphas, mask, p, q0, beta, lam, vpc)
        assert np.array_equal(got, again) and np.array_equal(pq, pq2), case
    record(f"regulariser {nx} x {ny} x {nz}: {nparts} partials, passes of the final loop: {_passes(nparts)}; min |partial| / "
           f"bound = {least:.2e} (needs {MARGIN:.0f}); <p,q> max |diff| / bound = {worst_pq:.2e} ((N + 16) eps), q {worst_q:.2e} "
           f"(16 eps sum |terms|)")


# ---------------------------------------------------------------------- the PCG kernels ---
PCG_CELLS = [65536,                       # 256 workgroups: the last size with one pass of k_pcg_scalar
             65537,                       # 257, the last with ONE cell
             ROUND,                       # 1024 workgroups, one round of the grid: four passes of k_pcg_scalar
             ROUND + 1,                   # one cell in the second round: the last one, and active
             2 * ROUND + 257]             # into the third round, with a ragged workgroup


def _pcg_blocks(ncell):
    return min(-(-ncell // 256), PCG_GRID)


def _block_sums(t, ncell):
    """t (vpc, ncell) longdouble terms -> the partial of every workgroup of ``k_pcg_update``: workgroup b takes the cells
    c with (c // 256) % blocks == b, of every vector of the column."""
    blocks = _pcg_blocks(ncell)
    s = np.concatenate([t.sum(axis=0), np.zeros(-ncell % 256, dtype=LD)]).reshape(-1, 256).sum(axis=1)
    return np.concatenate([s, np.zeros(-len(s) % blocks, dtype=LD)]).reshape(-1, blocks).sum(axis=0)


def _pcg_inputs(ncell, jacobi, first):
    K, vpc = 3, 2
    N = vpc * ncell
    rng = np.random.default_rng(ncell + 7 * K + jacobi + 2 * first)
    x, r, p, q = rng.uniform(0.5, 1.5, (4, K, vpc, ncell))
    hd, rd = (rng.uniform(0.5, 2.0, (vpc, ncell)), rng.uniform(0.1, 1.0, ncell)) if jacobi else (None, None)
    act = rng.uniform(size=ncell) < 0.8
    act[-1] = True                                               # the one cell of the last workgroup / round
    table = np.zeros((K, 8))
    table[:, 0] = 10 ** rng.uniform(-1, 1, K)
    table[:, 1] = 10.0 * N                                       # <b,b>: <r,r> of about N is far from tol^2 <b,b>
    table[:, 2] = rng.uniform(0.5, 2.0, K) * N                   # <r,z> of the iteration before: beta of order one
    table[:, 6] = 4
    pq = rng.uniform(0.5, 2.0, K) * 50 * N                       # alpha of about 1 / 50
    return K, vpc, N, x, r, p, q, hd, rd, act, table, pq


def _sum_condition(rn, z, ncell, N):
    """The partials of <r,z> and <r,r> per workgroup from the reference's new r and z: (bounds, least ratio)."""
    out = []
    for t in (rn * z, rn * rn):
        part, bound = _block_sums(t, ncell), (N + 16) * EPS * float(np.sum(np.abs(t)))
        assert len(part) == _pcg_blocks(ncell)
        assert np.min(np.abs(part)) >= MARGIN * bound            # the inputs: no workgroup's share can hide
        assert np.sum(np.abs(t[:, -1])) >= MARGIN * bound        # nor can the last cell on its own
        out.append(float(np.min(np.abs(part)) / bound))
    return min(out)


@pytest.mark.gpu
@pytest.mark.parametrize('jacobi', [True, False])
@pytest.mark.parametrize('ncell', PCG_CELLS)
def test_pcg_iteration_past_one_pass(ncell, jacobi):
    """update -> scalar -> direction with K = 3 columns of two vectors. The assertions of ``test_pcg_kernels_vs_numpy``:
    every element of x, r and p within 4 eps of the magnitudes, both sums within ``(N + 16) eps sum |terms|``, every
    entry of the table; column 1 is frozen and column 2 has <p,q> <= 0: x, r, p keep their bits. Column 0 must go on
    (state 0), so that the direction is formed. Before that, from the reference alone: the share of every workgroup in
    both sums, and that of the last cell, is at least 100 bounds. Twice: the same bits."""
    K, vpc, N, x, r, p, q, hd, rd, act, table, pq = _pcg_inputs(ncell, jacobi, 0)
    tol = 1e-3
    table[1, 7] = 1.0
    pq[2] = -0.25
    assert _lib.lib().emg3d_pcg_ws_len(ncell, K) == K * _pcg_blocks(ncell) * 2
    lam, rz0 = table[0, 0], table[0, 2]
    alpha = rz0 / pq[0]
    want_r = np.where(act, r[0] - LD(alpha) * q[0], 0)
    least = _sum_condition(want_r, _z_numpy(want_r, act, hd, rd, lam), ncell, N)
    got = _pcg(ncell, vpc, K, 0, x, r, p, q, hd, rd, act, table, pq, tol)
    gx, gr, gp = (a.reshape(K, vpc, ncell) for a in got[:3])
    gt = got[3]
    assert not np.any(np.isnan(gx)) and not np.any(np.isnan(gr)) and not np.any(np.isnan(gp))
    for k in (1, 2):
        assert np.array_equal(gx[k], x[k]) and np.array_equal(gr[k], r[k]) and np.array_equal(gp[k], p[k])
        assert gt[k, 7] == k and gt[k, 6] == 4 and gt[k, 2] == table[k, 2]
    assert gt[2, 4] == pq[2]
    assert np.all(np.abs(gx[0] - (x[0] + LD(alpha) * p[0])) <= 4 * EPS * (np.abs(x[0]) + np.abs(alpha * p[0])))
    assert np.all(np.abs(gr[0] - want_r) <= 4 * EPS * (np.abs(r[0]) + np.abs(alpha * q[0])))
    assert np.all(gr[0][:, ~act] == 0.0)
    z = _z_numpy(gr[0], act, hd, rd, lam)
    rz, rr = np.sum(gr[0] * z), np.sum(gr[0].astype(LD) ** 2)
    brz, brr = (N + 16) * EPS * np.sum(np.abs(gr[0] * z)), (N + 16) * EPS * rr
    worst = max(float(abs(gt[0, 2] - rz) / brz), float(abs(gt[0, 5] - rr) / brr))
    record(f"pcg iteration n={ncell} K={K} jacobi={jacobi}: {_pcg_blocks(ncell)} partials, passes of the final loop: "
           f"{_passes(_pcg_blocks(ncell))}, rounds of the grid: {-(-ncell // ROUND)}; min |partial| / bound = {least:.2e} (needs "
           f"{MARGIN:.0f}); sums max |diff| / bound = {worst:.2e} ((N + 16) eps)")
    assert abs(gt[0, 2] - rz) <= brz and abs(gt[0, 5] - rr) <= brr
    assert gt[0, 3] == rz0 and gt[0, 4] == pq[0] and gt[0, 6] == 5 and gt[0, 0] == lam and gt[0, 1] == table[0, 1]
    assert not gt[0, 5] <= tol * tol * gt[0, 1]                  # the table's own sums: not converged,
    assert gt[0, 7] == 0                                         # so the direction is formed
    beta = gt[0, 2] / gt[0, 3]
    assert np.all(np.abs(gp[0] - (z + LD(beta) * p[0])) <= 4 * EPS * (np.abs(z) + np.abs(beta * p[0])))
    again = _pcg(ncell, vpc, K, 0, x, r, p, q, hd, rd, act, table, pq, tol)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


@pytest.mark.gpu
@pytest.mark.parametrize('jacobi', [True, False])
@pytest.mark.parametrize('ncell', PCG_CELLS)
def test_pcg_setup_past_one_pass(ncell, jacobi):
    """The set-up (``first = 1``) as ``test_pcg_kernels_vs_numpy`` has it: r holds b, which is masked and summed, p = z;
    the last column has b = 0 and is frozen at once (state 1, p not touched). x, p and q are NaN before the call. The
    condition on the workgroups' shares is asserted for the two columns that have any. Twice: the same bits."""
    K, vpc, N, x, b, p, q, hd, rd, act, table, pq = _pcg_inputs(ncell, jacobi, 1)
    tol = 1e-3
    b[K - 1] = 0.0
    first = np.zeros((K, 8))
    first[:, 0] = table[:, 0]
    nan = np.full_like(x, np.nan)
    least = min(_sum_condition(np.where(act, b[k], 0).astype(LD), _z_numpy(np.where(act, b[k], 0), act, hd, rd, first[k, 0]),
                               ncell, N) for k in range(K - 1))
    got = _pcg(ncell, vpc, K, 1, nan, b, nan, nan, hd, rd, act, first, np.full(K, np.nan), tol)
    fr, fp, ft = got[1].reshape(K, vpc, ncell), got[2].reshape(K, vpc, ncell), got[3]
    assert np.all(np.isnan(got[0]))                              # x is not touched by the set-up
    worst = 0.0
    for k in range(K):
        assert np.array_equal(fr[k], np.where(act, b[k], 0.0))
        z = _z_numpy(fr[k], act, hd, rd, first[k, 0])
        rr, rz = np.sum(fr[k].astype(LD) ** 2), np.sum(fr[k] * z)
        assert abs(ft[k, 5] - rr) <= (N + 16) * EPS * rr and ft[k, 1] == ft[k, 5] and ft[k, 6] == 0
        assert abs(ft[k, 2] - rz) <= (N + 16) * EPS * np.sum(np.abs(fr[k] * z))
        assert ft[k, 0] == first[k, 0] and ft[k, 3] == 0 and ft[k, 4] == 0
        if k == K - 1:
            assert rr == 0 and ft[k, 7] == 1 and np.all(np.isnan(fp[k]))          # frozen at once: p is not touched
        else:
            worst = max(worst, float(abs(ft[k, 5] - rr) / ((N + 16) * EPS * rr)),
                        float(abs(ft[k, 2] - rz) / ((N + 16) * EPS * np.sum(np.abs(fr[k] * z)))))
            assert ft[k, 7] == 0 and np.all(np.abs(fp[k] - z) <= 4 * EPS * np.abs(z))
    record(f"pcg set-up n={ncell} K={K} jacobi={jacobi}: {_pcg_blocks(ncell)} partials, passes of the final loop: "
           f"{_passes(_pcg_blocks(ncell))}, rounds of the grid: {-(-ncell // ROUND)}; min |partial| / bound = {least:.2e} (needs "
           f"{MARGIN:.0f}); sums max |diff| / bound = {worst:.2e} ((N + 16) eps)")
    again = _pcg(ncell, vpc, K, 1, nan, b, nan, nan, hd, rd, act, first, np.full(K, np.nan), tol)
    assert all(np.array_equal(a, c, equal_nan=True) for a, c in zip(got, again))


# ------------------------------------------------------------------- eta_is_imaginary ---
ETA_SHAPES = [(64, 64, 64),               # 262 144 cells: one round of 1024 x 256 exactly
              (65, 64, 64),               # into the second
              (128, 64, 65)]              # into the third
ETA_LAYOUTS = {'three arrays': (0, 1, 2), 'one array for all three': (0, 0, 0), 'eta_y is eta_x': (0, 0, 2)}
TINY = 1e-300                             # a real part: anything that is not 0


def _is_imaginary(shape, is_complex, eta):
    """``emg3d_dev_eta_is_imaginary`` on a level filled by hand: it reads nx, ny, nz, is_complex and the three eta."""
    from emg3d_amd._device import _ptr, _stream
    lv = _lib.Level()
    lv.nx, lv.ny, lv.nz = shape
    lv.is_complex = int(is_complex)
    lv.eta_x, lv.eta_y, lv.eta_z = (None if t is None else _ptr(t) for t in eta)
    res = ctypes.c_int(-7)                                       # must be WRITTEN
    _lib.check(_lib.lib().emg3d_dev_eta_is_imaginary(ctypes.byref(lv), ctypes.byref(res), _stream()),
               'emg3d_dev_eta_is_imaginary')
    return res.value


@pytest.mark.gpu
@pytest.mark.parametrize('layout', list(ETA_LAYOUTS))
@pytest.mark.parametrize('shape', ETA_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_eta_is_imaginary_past_one_round(shape, layout):
    """All-imaginary eta: 1. ONE real part of 1e-300 -- at index 0, at the last index of the first round of the grid, at
    the first of the second, at the last cell; in each distinct array of the layout in turn --: 0, and 1 again once it
    is taken back. Behind the n cells of every array lie values WITH a real part, which must not be read. A real level:
    0. The answer sets ``EMG3D_LEVEL_ETA_IMAG`` for a whole hierarchy: a real part missed in a late cell would make the
    point smoother store half of every record, and nothing would report it."""
    n = shape[0] * shape[1] * shape[2]
    rng = np.random.default_rng(n)
    fence = np.full(5, 1.0 + 1.0j)
    arrays = [_up(np.concatenate([1j * rng.uniform(0.5, 1.5, n), fence])) for _ in range(3)]
    eta = [arrays[i] for i in ETA_LAYOUTS[layout]]
    places = sorted({0, ROUND - 1, ROUND, n - 1} & set(range(n)))
    assert _is_imaginary(shape, True, eta) == 1 and _is_imaginary(shape, True, eta) == 1
    found = 0
    for i in sorted(set(ETA_LAYOUTS[layout])):
        for place in places:
            arrays[i][place] = complex(TINY, 1.0)
            assert _is_imaginary(shape, True, eta) == 0, (i, place)
            assert _is_imaginary(shape, True, eta) == 0, (i, place)
            arrays[i][place] = complex(0.0, 1.0)
            assert _is_imaginary(shape, True, eta) == 1, (i, place)
            found += 1
    assert _is_imaginary(shape, False, eta) == 0 and _is_imaginary(shape, False, [None] * 3) == 0
    record(f"eta_is_imaginary {shape} {layout}: {n} cells, rounds of the grid: {-(-n // ROUND)}; one real part of {TINY} found "
           f"at each of {places} in each of {len(set(ETA_LAYOUTS[layout]))} arrays ({found} calls)")
