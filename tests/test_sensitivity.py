"""Sensitivity products: ``emg3d_dev_sensitivity_source`` (the operator G of ``Simulation.jvec``,
emg3d/simulations.py:1352-1362) and ``gradient.Sensitivity`` / ``jvec`` / ``jtvec`` with kept forward fields.

The kernel's arithmetic is checked against a NumPy restatement of G in this file (``G_numpy``), which is itself
pinned to reference-computed arrays (``tests/golden/gradient.npz``) on the CPU through the kernel-level identity

    sum_cells v_k * gradient_accumulate(e, b)_k == -Re sum_edges b * sensitivity_source(e, v)               (B)

and the whole operators through

    sum(v * jtvec(y)) == Re sum_i conj(y_i) * jvec(v)_i           for real v, complex y                      (A)

Figures that the GPU tests observe are printed, and appended to the file named by the environment variable
``EMG3D_AMD_PARITY_FILE`` when it is set (``profiles/sensitivity_parity.txt`` is such a run).
"""
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest

import emg3d_amd as emg3d
from emg3d_amd import _lib, gradient
from helpers import widths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU_0 = 1.25663706127e-06          # as emg3d_amd.fields (scipy.constants.mu_0)
EPS = np.finfo(float).eps


def record(line):
    print(line)
    path = os.environ.get('EMG3D_AMD_PARITY_FILE')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


# ------------------------------------------------------------------------ the checker ---
def cells_to_edges(w3):
    """(3, nx, ny, nz) cell values -> the sums over the (up to four) cells that share an edge, / 4, for the x-, y-
    and z-edges; cells added in the order lower z first, then lower y, then lower x."""
    _, nx, ny, nz = w3.shape
    ax, ay, az = np.zeros((nx, ny + 1, nz + 1)), np.zeros((nx + 1, ny, nz + 1)), np.zeros((nx + 1, ny + 1, nz))
    for d2 in (1, 0):             # offset 1: the edge's LOWER neighbour cell
        for d1 in (1, 0):
            ax[:, d1:ny + d1, d2:nz + d2] += w3[0]
            ay[d1:nx + d1, :, d2:nz + d2] += w3[1]
            az[d1:nx + d1, d2:ny + d2, :] += w3[2]
    return ax / 4, ay / 4, az / 4


def G_numpy(e, v3, volumes, smu0):
    """G v = -s mu0 * e * cells_to_edges(volumes * v): field-shaped vector [gx | gy | gz] (F-order)."""
    a = np.concatenate([c.ravel('F') for c in cells_to_edges(volumes[None] * v3)])
    return -smu0 * e * a


# ----------------------------------------------------------------------- not gpu tests ---
def test_checker_is_pinned_to_the_reference(golden_gradient):
    """(B) with the reference's own arrays: ``grad_cells_raw`` is what the reference's gradient forms from
    ``efield`` and ``bfield`` (real(bfield s mu0 efield), edges -> cells with volumes). Bound 1e-13 relative:
    both sides are sums of ~3 500 fp64 terms (sqrt(N) eps ~ 1e-14 for random signs)."""
    g = golden_gradient
    grid = emg3d.TensorMesh([g['hx'], g['hy'], g['hz']], g['origin'])
    smu0 = 2j * np.pi * float(g['frequency']) * float(g['meta_mu_0'])
    v = np.random.default_rng(0).standard_normal((3,) + tuple(grid.shape_cells))
    vol = grid.cell_volumes.reshape(grid.shape_cells, order='F')
    lhs = np.sum(v * g['grad_cells_raw'])
    rhs = -np.sum(g['bfield'] * G_numpy(g['efield'], v, vol, smu0)).real
    rel = abs(lhs - rhs) / abs(lhs)
    print(f"(B) vs reference arrays: lhs {lhs:.16e} rhs {rhs:.16e} rel {rel:.2e}")
    assert rel <= 1e-13


def small_model(case='isotropic', mapping='Resistivity', seed=3):
    hx, hz = widths(4, 3, 50., 1.3), widths(4, 2, 40., 1.3)
    grid = emg3d.TensorMesh([hx, hx, hz], (-hx.sum() / 2, -hx.sum() / 2, -hz[:4].sum()))
    rng = np.random.default_rng(seed)
    n = gradient._NCOMP[case]
    rho = [10 ** rng.uniform(-0.2, 0.5, grid.shape_cells) for _ in range(n)]
    to = {'Resistivity': lambda r: r, 'Conductivity': lambda r: 1 / r, 'LgResistivity': np.log10,
          'LgConductivity': lambda r: -np.log10(r), 'LnResistivity': np.log, 'LnConductivity': lambda r: -np.log(r)}
    props = [to[mapping](r) for r in rho]
    names = {'isotropic': ('property_x',), 'HTI': ('property_x', 'property_y'), 'VTI': ('property_x', 'property_z'),
             'triaxial': ('property_x', 'property_y', 'property_z')}[case]
    return grid, emg3d.Model(grid, mapping=mapping, **dict(zip(names, props)))


SRCS = {'a': (-60., 0., -30., 0., 0.), 'b': (40., 30., -30., 90., 0.)}
FREQS = {'f': 1.0}
RECS = np.array([[70., 10., -40., 0., 0.], [-30., -60., -40., 90., 0.], [10., 80., -25., 45., 0.]])


def test_public_names_and_declared_symbol():
    from emg3d_amd.gradient import Sensitivity, jvec, jtvec       # noqa: F401
    assert 'emg3d_dev_sensitivity_source' in _lib.SIGNATURES
    assert hasattr(_lib.lib(), 'emg3d_dev_sensitivity_source')
    for name in ('Sensitivity', 'jvec', 'jtvec'):
        assert name in gradient.__all__


@pytest.mark.parametrize('case, n', [('isotropic', 1), ('HTI', 2), ('VTI', 2), ('triaxial', 3)])
def test_vector_shape_is_validated_before_any_gpu_work(case, n):
    grid, model = small_model(case)
    shape = tuple(grid.shape_cells)
    lin = gradient.Sensitivity(model, SRCS, FREQS, RECS)
    for bad in ((n + 1,) + shape, shape[:2], (n,) + shape[::-1][:2] + (3,)) + (() if n == 1 else (shape,)):
        with pytest.raises(ValueError, match=r"`vector` must be real with shape .*%d, %d, %d\)" % shape):
            lin.jvec(np.zeros(bad))
    with pytest.raises(ValueError, match="must be real"):
        lin.jvec(np.zeros((n,) + shape, dtype=complex))
    with pytest.raises(ValueError, match="one value per receiver"):
        lin.jtvec({('a', 'f'): np.zeros(len(RECS) + 1, dtype=complex)})
    good = gradient.expand_vector(model, np.ones((n,) + shape))
    assert good.shape == (3,) + shape
    if n == 1:
        assert np.array_equal(good, gradient.expand_vector(model, np.ones(shape)))


def test_epsilon_r_and_mu_r_are_refused():
    grid, model = small_model()
    ones = np.ones(grid.shape_cells)
    for kw, name in (({'epsilon_r': 2 * ones}, 'el. permittivity'), ({'mu_r': 2 * ones}, 'magn. permeability')):
        m = emg3d.Model(grid, property_x=ones, **kw)
        with pytest.raises(NotImplementedError, match=f"Gradient not implemented for {name}"):
            gradient.Sensitivity(m, SRCS, FREQS, RECS)
        with pytest.raises(NotImplementedError, match=name):
            gradient.jvec(m, ones, SRCS, FREQS, RECS)
        with pytest.raises(NotImplementedError, match=name):
            gradient.jtvec(m, {}, SRCS, FREQS, RECS)
    gradient.Sensitivity(emg3d.Model(grid, property_x=ones, epsilon_r=ones, mu_r=ones), SRCS, FREQS, RECS)
    with pytest.raises(ValueError, match="`keep` must be"):
        gradient.Sensitivity(model, SRCS, FREQS, RECS, keep='disk')


def test_expansion_by_anisotropy_case():
    """(v, v, v) / (v0, v1, v0) / (v0, v0, v1) / as given (emg3d/simulations.py:1340-1349); with the mapping
    'Conductivity' the derivative chain is the identity."""
    rng = np.random.default_rng(1)
    for case, pick in (('isotropic', (0, 0, 0)), ('HTI', (0, 1, 0)), ('VTI', (0, 0, 1)), ('triaxial', (0, 1, 2))):
        grid, model = small_model(case, 'Conductivity')
        v = rng.standard_normal((len(set(pick)),) + tuple(grid.shape_cells))
        out = gradient.expand_vector(model, v)
        for k in range(3):
            assert np.array_equal(out[k], v[pick[k]]), (case, k)


def test_derivative_chain_of_the_six_mappings():
    """d sigma / d property, written out by hand (emg3d/maps.py:120-330), applied to the vector BEFORE G."""
    ln10 = np.log(10.0)
    expected = {'Conductivity': lambda p: np.ones_like(p), 'Resistivity': lambda p: -1 / p ** 2,
                'LgConductivity': lambda p: ln10 * 10 ** p, 'LgResistivity': lambda p: -ln10 * 10 ** -p,
                'LnConductivity': lambda p: np.exp(p), 'LnResistivity': lambda p: -np.exp(-p)}
    rng = np.random.default_rng(2)
    for mapping, dsigma in expected.items():
        grid, model = small_model('triaxial', mapping)
        v = rng.standard_normal((3,) + tuple(grid.shape_cells))
        out = gradient.expand_vector(model, v)
        for k, p in enumerate((model.property_x, model.property_y, model.property_z)):
            assert np.allclose(out[k], v[k] * dsigma(p), rtol=1e-14, atol=0), (mapping, k)
        # ... and it is the derivative of the mapping: central differences of sigma(p)
        p = np.asarray(model.property_x)
        sig = {'Conductivity': lambda q: q, 'Resistivity': lambda q: 1 / q, 'LgConductivity': lambda q: 10 ** q,
               'LgResistivity': lambda q: 10 ** -q, 'LnConductivity': np.exp, 'LnResistivity': lambda q: np.exp(-q)}[mapping]
        d = 1e-6
        assert np.allclose((sig(p + d) - sig(p - d)) / (2 * d), dsigma(p), rtol=1e-7)


def test_no_cpu_fallback_without_gpu():
    if _lib.lib().emg3d_device_count() > 0:
        pytest.skip("GPU present")
    grid, model = small_model()
    lin = gradient.Sensitivity(model, SRCS, FREQS, RECS)              # needs no device
    assert "2 pairs" in repr(lin) and lin.n_solves == {'forward': 0, 'jvec': 0, 'jtvec': 0}
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        lin.jvec(np.ones(grid.shape_cells))
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        lin.jtvec({('a', 'f'): np.ones(3, dtype=complex)})
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        gradient.jvec(model, np.ones(grid.shape_cells), SRCS, FREQS, RECS)
    with pytest.raises(_lib.Emg3dAmdError, match="no HIP device"):
        lin.synthetic


# --------------------------------------------------------------------------- gpu tests ---
def _run_kernel(grid, e, v3, smu0, alias):
    """emg3d_dev_sensitivity_source through ctypes; ``alias``: vy and vz are the SAME buffer as vx."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    dev = torch.device('cuda', torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    nx, ny, nz = grid.shape_cells
    o1, o2 = grid.n_edges_x, grid.n_edges_x + grid.n_edges_y
    ed, vol = up(e), up(grid.cell_volumes.astype(np.float64))
    vd = [up(c.ravel('F')) for c in v3]
    if alias:
        vd = [vd[0]] * 3
    out = torch.full((grid.n_edges,), float('nan'), dtype=ed.dtype, device=dev)       # every edge must be WRITTEN
    _lib.check(_lib.lib().emg3d_dev_sensitivity_source(
        nx, ny, nz, int(np.iscomplexobj(e)), _ptr(ed), _ptr(ed, o1), _ptr(ed, o2), complex(smu0).real, complex(smu0).imag,
        _ptr(vol), _ptr(vd[0]), _ptr(vd[1]), _ptr(vd[2]), _ptr(out), _ptr(out, o1), _ptr(out, o2), _stream()),
        'emg3d_dev_sensitivity_source')
    return out.cpu().numpy()


def _stretched(nx, ny, nz):
    h = [30. * 1.07 ** np.abs(np.arange(n) - n / 3) for n in (nx, ny, nz)]
    return emg3d.TensorMesh(h, (-10., 5., -200.))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(67, 5, 9), (12, 10, 8)])
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('alias', [True, False])
def test_kernel_vs_numpy_restatement(shape, is_complex, alias):
    """Entry by entry against ``G_numpy`` within ``8 eps |s mu0| |e| (sum |w| / 4)``, w = volume * v over the
    edge's cells: a bound on the magnitude of the FACTORS, not of the result -- the two real products of a complex
    multiplication can cancel. Both sides do a handful of fp64 operations per entry (three additions, the products
    volume * v -- fused into the additions in the library, rounded separately by NumPy --, a complex and a real
    multiplication): at most ~7 roundings of eps / 2 on either side, 7 eps between them in the worst case."""
    grid = _stretched(*shape)
    rng = np.random.default_rng(sum(shape) + 2 * is_complex + alias)
    n = grid.n_edges
    e = rng.standard_normal(n) + (1j * rng.standard_normal(n) if is_complex else 0)
    v3 = rng.standard_normal((3,) + shape)
    if alias:
        v3[1:] = v3[0]
    smu0 = 2j * np.pi * 0.7 * MU_0 if is_complex else 0.7 * MU_0         # Laplace domain: s = -f real, fields real
    vol = grid.cell_volumes.reshape(shape, order='F')
    got = _run_kernel(grid, e, v3, smu0, alias)
    want = G_numpy(e, v3, vol, smu0)
    if not is_complex:
        assert got.dtype == np.float64
        want = want.real
    mag = np.concatenate([c.ravel('F') for c in cells_to_edges(np.abs(vol[None] * v3))])
    bound = 8 * EPS * abs(smu0) * np.abs(e) * mag
    assert not np.any(np.isnan(got))
    worst = float(np.max(np.abs(got - want) / bound))
    record(f"kernel vs NumPy {shape} complex={is_complex} alias={alias}: max |diff| / bound = {worst:.3f} (bound 8 eps)")
    assert np.all(np.abs(got - want) <= bound)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(67, 5, 9), (12, 10, 8)])
def test_kernel_is_the_transpose_of_gradient_accumulate(shape):
    """(B) on the device, against emg3d_dev_gradient_accumulate itself: <= 1e-13 relative (sums of ~1e4 terms)."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    grid = _stretched(*shape)
    rng = np.random.default_rng(11)
    n, nc = grid.n_edges, grid.n_cells
    e = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    v3 = rng.uniform(0.5, 1.5, (3,) + shape)
    smu0 = 2j * np.pi * 0.7 * MU_0
    dev = torch.device('cuda', torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    ed, bd, vol = up(e), up(b), up(grid.cell_volumes.astype(np.float64))
    g = torch.zeros(3 * nc, dtype=torch.float64, device=dev)
    o1, o2 = grid.n_edges_x, grid.n_edges_x + grid.n_edges_y
    _lib.check(_lib.lib().emg3d_dev_gradient_accumulate(
        *shape, 1, _ptr(ed), _ptr(ed, o1), _ptr(ed, o2), _ptr(bd), _ptr(bd, o1), _ptr(bd, o2), smu0.real, smu0.imag,
        _ptr(vol), _ptr(g), _ptr(g, nc), _ptr(g, 2 * nc), _stream()), 'emg3d_dev_gradient_accumulate')
    lhs = float(np.sum(np.concatenate([c.ravel('F') for c in v3]) * g.cpu().numpy()))
    rhs = -float(np.sum(b * _run_kernel(grid, e, v3, smu0, False)).real)
    rel = abs(lhs - rhs) / abs(lhs)
    record(f"(B) on the device {shape}: lhs {lhs:.16e} rhs {rhs:.16e} rel {rel:.2e} (bound 1e-13)")
    assert rel <= 1e-13


@pytest.mark.gpu
def test_bad_pointers_are_refused():
    with pytest.raises(_lib.Emg3dAmdError, match="sensitivity_source: bad argument"):
        _lib.check(_lib.lib().emg3d_dev_sensitivity_source(4, 4, 4, 1, None, None, None, 0., 1., None, None, None,
                                                           None, None, None, None, None), 'emg3d_dev_sensitivity_source')


TOL = 1e-10
OPTS = dict(tol=TOL, sslsolver=True)


def _inner(y, jv):
    return float(sum(np.sum(np.conj(y[k]) * jv[k]).real for k in y))


def _random_data(rng, pairs, nrec):
    return {p: rng.standard_normal(nrec) + 1j * rng.standard_normal(nrec) for p in pairs}


def _maxdiff(a, b):
    """Largest difference of two data dicts / arrays relative to the max-norm of the second."""
    if isinstance(a, dict):
        assert list(a) == list(b)
        a, b = np.concatenate([a[k] for k in a]), np.concatenate([b[k] for k in b])
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


ADJOINT_CASES = {
    'isotropic-resistivity': dict(case='isotropic', mapping='Resistivity'),
    'HTI': dict(case='HTI', mapping='Resistivity'),
    'VTI': dict(case='VTI', mapping='Conductivity'),
    'triaxial-LgResistivity': dict(case='triaxial', mapping='LgResistivity'),
    'computational-grid': dict(case='isotropic', mapping='Conductivity', comp=True),
    'magnetic-receiver': dict(case='isotropic', mapping='Resistivity', magnetic=[False, True, False]),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(ADJOINT_CASES))
def test_jvec_and_jtvec_are_adjoint(name):
    """(A) for random real v and random COMPLEX y, all solves at tol 1e-10; criterion of the reference's own test
    (discretize.tests.assert_isadjoint, relative 1e-6; tests/test_simulations.py:880-970)."""
    spec = ADJOINT_CASES[name]
    grid, model = small_model(spec['case'], spec['mapping'])
    kw = {}
    if spec.get('comp'):
        cx, cz = widths(6, 3, 35., 1.25), widths(6, 3, 28., 1.25)
        kw['grids'] = emg3d.TensorMesh([cx, cx, cz], (-cx.sum() / 2, -cx.sum() / 2, -cz[:6].sum()))
    lin = gradient.Sensitivity(model, SRCS, FREQS, RECS, solver_opts=OPTS, tol_gradient=TOL,
                               magnetic=spec.get('magnetic'), **kw)
    rng = np.random.default_rng(17)
    n = gradient._NCOMP[spec['case']]
    v = rng.standard_normal((n,) + tuple(grid.shape_cells))
    y = _random_data(rng, lin.pairs, len(RECS))
    jv = lin.jvec(v)
    jt = lin.jtvec(y)
    assert jt.shape == ((n,) + tuple(grid.shape_cells) if n > 1 else tuple(grid.shape_cells))
    assert all(jv[p].shape == (len(RECS),) and np.iscomplexobj(jv[p]) for p in lin.pairs)
    lhs, rhs = float(np.sum(v.reshape(jt.shape) * jt)), _inner(y, jv)
    rel = abs(lhs - rhs) / min(abs(lhs), abs(rhs))
    record(f"(A) {name}: sum(v jtvec(y)) {lhs:.12e}  Re sum conj(y) jvec(v) {rhs:.12e}  rel {rel:.2e} (bound 1e-6)")
    assert lin.n_solves == {'forward': 2, 'jvec': 2, 'jtvec': 2}
    assert rel <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize('case, mapping', [('isotropic', 'Resistivity'), ('VTI', 'LgConductivity')])
def test_jvec_is_the_derivative_of_the_responses(case, mapping):
    """Taylor remainders of the responses F along a random direction v in the model's own mapping, for three steps h
    a decade apart: with the jvec term they fall with order >= 1.7 (expected 2; 0.85 x 2 is the criterion of the
    reference's check_derivative), without it with order < 1.3 (expected 1) -- the test discriminates. Solves at
    1e-12 keep the smallest remainder (~1e-7 of |F| x curvature) far above solver noise."""
    grid, model = small_model(case, mapping)
    opts = dict(tol=1e-12, sslsolver=True)
    names = [k for k in ('property_x', 'property_y', 'property_z') if getattr(model, k) is not None]
    rng = np.random.default_rng(23)
    # a relative perturbation of the conductivities of ~ h in either mapping (log10 mapping: d lg sigma = h / ln 10)
    scale = [np.asarray(getattr(model, k)) if mapping == 'Resistivity' else np.full(grid.shape_cells, 1 / np.log(10))
             for k in names]
    v = np.stack([s * rng.standard_normal(grid.shape_cells) for s in scale])

    def responses(m):
        lin = gradient.Sensitivity(m, SRCS, FREQS, RECS, solver_opts=opts, tol_gradient=1e-12)
        syn = lin.synthetic
        return lin, np.concatenate([syn[p] for p in lin.pairs])
    lin, f0 = responses(model)
    jv = lin.jvec(v if len(names) > 1 else v[0])
    jv = np.concatenate([jv[p] for p in lin.pairs])
    steps = (3e-2, 3e-3, 3e-4)
    r_with, r_without = [], []
    for h in steps:
        moved = emg3d.Model(grid, mapping=mapping, **{k: np.asarray(getattr(model, k)) + h * v[i]
                                                        for i, k in enumerate(names)})
        fh = responses(moved)[1]
        r_without.append(float(np.linalg.norm(fh - f0)))
        r_with.append(float(np.linalg.norm(fh - f0 - h * jv)))
    o_with = [np.log10(r_with[i] / r_with[i + 1]) for i in range(2)]
    o_without = [np.log10(r_without[i] / r_without[i + 1]) for i in range(2)]
    record(f"Taylor {case}/{mapping}: h {steps}  |F| {np.linalg.norm(f0):.3e}  remainders with jvec "
           f"{', '.join(f'{r:.3e}' for r in r_with)} (orders {o_with[0]:.3f}, {o_with[1]:.3f}; bound >= 1.7)  without "
           f"{', '.join(f'{r:.3e}' for r in r_without)} (orders {o_without[0]:.3f}, {o_without[1]:.3f}; bound < 1.3)")
    assert all(o >= 1.7 for o in o_with)
    assert all(o < 1.3 for o in o_without)


def _fd_inputs():
    """The inputs of test_gpu_parity.test_adjoint_gradient_vs_finite_differences."""
    rng = np.random.default_rng(3)
    hx, hz = widths(4, 3, 50., 1.3), widths(4, 2, 40., 1.3)
    grid = emg3d.TensorMesh([hx, hx, hz], (-hx.sum() / 2, -hx.sum() / 2, -hz[:4].sum()))
    shape = grid.shape_cells
    rho = 10 ** rng.uniform(-0.2, 0.5, shape)
    true = emg3d.Model(grid, property_x=rho * (1 + 0.3 * rng.standard_normal(shape) * 0.5).clip(0.5, 2.0))
    obs = {}
    for s in SRCS:
        ef = emg3d.solve(true, emg3d.get_source_field(grid, SRCS[s], 1.0), **OPTS)
        obs[(s, 'f')] = emg3d.fields.get_receiver(ef, tuple(RECS[:, k] for k in range(5)), 'linear')
    wts = {k: 1.0 / (0.05 * np.abs(v)) ** 2 for k, v in obs.items()}
    return grid, emg3d.Model(grid, property_x=rho), obs, wts


@pytest.mark.gpu
def test_jtvec_of_the_weighted_residual_is_the_gradient():
    """``lin.misfit_and_gradient`` and ``lin.jtvec(residual * weights)`` against the existing function: misfit to
    1e-12 relative, gradient to 100 x tol of its max-norm (both converged to tol; the device source assembly uses
    atomic adds, bit-identity is not promised)."""
    grid, model, obs, wts = _fd_inputs()
    m0, g0, info0 = gradient.misfit_and_gradient(model, SRCS, FREQS, RECS, obs, wts, solver_opts=OPTS, tol_gradient=TOL)
    lin = gradient.Sensitivity(model, SRCS, FREQS, RECS, solver_opts=OPTS, tol_gradient=TOL)
    m1, g1 = lin.misfit_and_gradient(obs, wts)
    g2 = lin.jtvec({p: (lin.synthetic[p] - obs[p]) * wts[p] for p in lin.pairs})
    one = gradient.jtvec(model, {p: (lin.synthetic[p] - obs[p]) * wts[p] for p in lin.pairs}, SRCS, FREQS, RECS,
                         solver_opts=OPTS, tol_gradient=TOL)
    record(f"jtvec(residual w) vs misfit_and_gradient: misfit rel {abs(m1 - m0) / m0:.2e} (bound 1e-12); gradient "
           f"max-norm rel {_maxdiff(g1, g0):.2e}, {_maxdiff(g2, g0):.2e}, one-shot {_maxdiff(one, g0):.2e} (bound 1e-8); "
           f"bit-identical: {np.array_equal(g1, g0)}, {np.array_equal(g2, g0)}")
    assert set(info0[('a', 'f')]) == {'forward', 'backward', 'synthetic'}
    assert abs(m1 - m0) <= 1e-12 * m0
    for g in (g1, g2, one):
        assert g.shape == g0.shape and _maxdiff(g, g0) <= 100 * TOL
    assert lin.n_solves == {'forward': 2, 'jvec': 0, 'jtvec': 4}


@pytest.mark.gpu
def test_forward_fields_are_kept():
    """After ``forward()`` no call solves the forward problem again; 'host' holds the same bits as 'device';
    ``keep=False`` recomputes (equal within 100 x tol); ``release()`` frees the kept tensors."""
    import torch
    grid, model = small_model()
    rng = np.random.default_rng(29)
    v = rng.standard_normal(grid.shape_cells)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    lin = gradient.Sensitivity(model, SRCS, FREQS, RECS, solver_opts=OPTS, tol_gradient=TOL)
    y = _random_data(rng, lin.pairs, len(RECS))
    assert lin.forward() is lin and lin.n_solves == {'forward': 2, 'jvec': 0, 'jtvec': 0}
    assert lin.kept_bytes == 2 * grid.n_edges * 16 and f"{lin.kept_bytes:,} B" in repr(lin)
    jv = [lin.jvec(v * k) for k in (1, 2, 3)]
    jt = [lin.jtvec({p: y[p] * k for p in y}) for k in (1, 2, 3)]
    assert lin.n_solves == {'forward': 2, 'jvec': 6, 'jtvec': 6}
    held = torch.cuda.memory_allocated()
    kept = lin.kept_bytes
    lin.release()
    torch.cuda.synchronize()
    freed = held - torch.cuda.memory_allocated()
    record(f"release(): {freed:,} B freed, kept fields {kept:,} B; allocated before {before:,} B")
    assert freed >= kept and lin.kept_bytes == 0

    host = gradient.Sensitivity(model, SRCS, FREQS, RECS, solver_opts=OPTS, tol_gradient=TOL, keep='host')
    jvh, jth = host.jvec(v), host.jtvec(y)
    assert host.n_solves == {'forward': 2, 'jvec': 2, 'jtvec': 2}
    assert all(t.device.type == 'cpu' and t.is_pinned() for t in host._kept.values())
    assert all(np.array_equal(jvh[p], jv[0][p]) for p in jvh) and np.array_equal(jth, jt[0])

    none = gradient.Sensitivity(model, SRCS, FREQS, RECS, solver_opts=OPTS, tol_gradient=TOL, keep=False)
    jvn, jtn = none.jvec(v), none.jtvec(y)
    assert none.n_solves == {'forward': 4, 'jvec': 2, 'jtvec': 2} and none.kept_bytes == 0
    record(f"keep=False vs 'device': jvec {_maxdiff(jvn, jv[0]):.2e}, jtvec {_maxdiff(jtn, jt[0]):.2e} (bound 1e-8)")
    assert _maxdiff(jvn, jv[0]) <= 100 * TOL and _maxdiff(jtn, jt[0]) <= 100 * TOL
    one = gradient.jvec(model, v, SRCS, FREQS, RECS, solver_opts=OPTS, tol_gradient=TOL)
    assert _maxdiff(one, jv[0]) <= 100 * TOL


@pytest.mark.gpu
@pytest.mark.parametrize('sslsolver', [False, True])
def test_batched_products(sslsolver):
    """``batch=2``: multigrid bit-identical to pair by pair (the guarantee of ``solve_batch``); BiCGSTAB (each source
    its own iteration) within 100 x tol."""
    grid, model = small_model('VTI')
    opts = dict(tol=TOL, sslsolver=sslsolver)
    rng = np.random.default_rng(31)
    v = rng.standard_normal((2,) + tuple(grid.shape_cells))
    res = []
    for batch in (1, 2):
        lin = gradient.Sensitivity(model, SRCS, FREQS, RECS, solver_opts=opts, tol_gradient=TOL, batch=batch)
        y = _random_data(np.random.default_rng(37), lin.pairs, len(RECS))
        res.append((lin.jvec(v), lin.jtvec(y)))
        assert lin.n_solves == {'forward': 2, 'jvec': 2, 'jtvec': 2}
        assert [len(c) for c in lin._chunks()] == ([1, 1] if batch == 1 else [2])
    (jv1, jt1), (jv2, jt2) = res
    same = all(np.array_equal(jv1[p], jv2[p]) for p in jv1) and np.array_equal(jt1, jt2)
    record(f"batch=2 vs 1, sslsolver={sslsolver}: jvec {_maxdiff(jv2, jv1):.2e}, jtvec {_maxdiff(jt2, jt1):.2e}; "
           f"bit-identical: {same}")
    if sslsolver:
        assert _maxdiff(jv2, jv1) <= 100 * TOL and _maxdiff(jt2, jt1) <= 100 * TOL
    else:
        assert same


@pytest.mark.gpu
def test_linearity_and_the_zero_vector():
    grid, model = small_model('HTI')
    lin = gradient.Sensitivity(model, SRCS, FREQS, RECS, solver_opts=OPTS, tol_gradient=TOL)
    zero = lin.jvec(np.zeros((2,) + tuple(grid.shape_cells)))
    assert lin.n_solves == {'forward': 2, 'jvec': 0, 'jtvec': 0}
    assert all(np.array_equal(zero[p], np.zeros(len(RECS), dtype=complex)) for p in lin.pairs)
    rng = np.random.default_rng(41)
    v1, v2 = rng.standard_normal((2, 2) + tuple(grid.shape_cells))
    a, b = 0.7, -2.3
    j1, j2, j12 = lin.jvec(v1), lin.jvec(v2), lin.jvec(a * v1 + b * v2)
    combo = {p: a * j1[p] + b * j2[p] for p in j1}
    record(f"linearity: jvec(a v1 + b v2) vs a jvec(v1) + b jvec(v2): {_maxdiff(j12, combo):.2e} (bound 1e-8)")
    assert _maxdiff(j12, combo) <= 100 * TOL
    assert np.array_equal(lin.jtvec({}), np.zeros((2,) + tuple(grid.shape_cells)))       # no data: no solve
    assert lin.n_solves['jtvec'] == 0


_TWO_RANKS = r"""
import os, sys, pickle
import numpy as np
import torch, torch.distributed as dist
root = os.environ['EMG3D_TEST_ROOT']
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, 'tests'))
from emg3d_amd import gradient, parallel
import test_sensitivity as ts
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
torch.cuda.set_device(0)
dist.init_process_group('gloo', rank=rank, world_size=world)
grid, model, srcs, freqs, v, y, opts = ts._two_rank_inputs()
lin = gradient.Sensitivity(model, srcs, freqs, ts.RECS, solver_opts=opts, tol_gradient=opts['tol'])
res = {'jvec': lin.jvec(v), 'jtvec': lin.jtvec(y), 'synthetic': lin.synthetic, 'n_solves': lin.n_solves,
       'mine': [lin.pairs[i] for i in lin._mine], 'kept': len(lin._kept)}
with open(os.path.join(os.environ['EMG3D_TEST_OUT'], f'rank{rank}.pkl'), 'wb') as f:
    pickle.dump(res, f)
parallel.finalize()
"""


def _two_rank_inputs():
    grid, model = small_model('VTI')
    srcs = dict(SRCS, c=(0., -50., -30., 30., 0.))
    freqs = {'f1': 1.0, 'f2': 2.5}
    rng = np.random.default_rng(43)
    v = rng.standard_normal((2,) + tuple(grid.shape_cells))
    y = _random_data(rng, [(s, f) for s in srcs for f in freqs], len(RECS))
    return grid, model, srcs, freqs, v, y, dict(tol=1e-8, sslsolver=True)


@pytest.mark.gpu
def test_two_ranks_on_one_gpu(tmp_path):
    """Two ranks (gloo) on this box's one GPU, six pairs: both return the complete jvec dict and the all-reduced
    jtvec, equal to the single-process results within 100 x tol; every pair is solved on exactly one rank, which
    keeps its forward field."""
    script = tmp_path / 'two_ranks_sensitivity.py'
    script.write_text(_TWO_RANKS)
    env = dict(os.environ, EMG3D_TEST_ROOT=ROOT, EMG3D_TEST_OUT=str(tmp_path), HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('EMG3D_AMD_PARITY_FILE', None)
    sk = socket.socket(); sk.bind(('127.0.0.1', 0)); port = sk.getsockname()[1]; sk.close()      # noqa: E702
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                        '--master-addr', '127.0.0.1', '--master-port', str(port), str(script)],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = [pickle.load(open(tmp_path / f'rank{k}.pkl', 'rb')) for k in (0, 1)]
    grid, model, srcs, freqs, v, y, opts = _two_rank_inputs()
    lin = gradient.Sensitivity(model, srcs, freqs, RECS, solver_opts=opts, tol_gradient=opts['tol'])
    jv, jt, syn = lin.jvec(v), lin.jtvec(y), lin.synthetic
    assert sorted(res[0]['mine'] + res[1]['mine']) == sorted(lin.pairs) and len(res[0]['mine']) == 3
    for k in (0, 1):
        n = len(res[k]['mine'])
        assert res[k]['n_solves'] == {'forward': n, 'jvec': n, 'jtvec': n} and res[k]['kept'] == n
        assert list(res[k]['jvec']) == lin.pairs == list(res[k]['synthetic'])
        record(f"two ranks, rank {k}: jvec {_maxdiff(res[k]['jvec'], jv):.2e}, jtvec {_maxdiff(res[k]['jtvec'], jt):.2e}, "
               f"synthetic {_maxdiff(res[k]['synthetic'], syn):.2e} (bound 1e-6 = 100 x tol)")
        assert _maxdiff(res[k]['jvec'], jv) <= 100 * opts['tol']
        assert _maxdiff(res[k]['jtvec'], jt) <= 100 * opts['tol']
        assert _maxdiff(res[k]['synthetic'], syn) <= 100 * opts['tol']
    assert np.array_equal(res[0]['jtvec'], res[1]['jtvec'])
    assert all(np.array_equal(res[0]['jvec'][p], res[1]['jvec'][p]) for p in lin.pairs)
