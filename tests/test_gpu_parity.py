"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against

* the oracle in its four-colour order (per-sweep, tolerance 2e-12 rel-L2),
* the golden vectors generated from the reference itself (order-independent kernels,
  tolerance 1e-13; converged solves, tolerance 1e-8 rel-L2 as stated in BASELINE.json),
* the reference's own golden file (tests/golden/regression_small.npz),
* size-independent properties at BASELINE.json's full sizes (128^3 / 256^3): linearity
  and complex symmetry of the operator, fixed-point property of the smoothers.

Nothing here reads /root/reference; the oracle (oracle/) is used only as the checker.
"""
import os

import numpy as np
import pytest
import torch

import emg3d_amd as emg3d
from emg3d_amd import core, solver, _lib
from emg3d_amd._device import DeviceLevel, _stream
from oracle import core as ocore
from oracle import mg_ref
from helpers import (admissible_sc_dirs, coarse_grid, pec_mask, random_field, random_level, relerr, sc_factors,
                     widths)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _oracle_threads():
    """The oracle's four-colour / tiled orders walk classes of independent nodes, lines and tiles: with threads
    (oracle_set_threads) the values are the same bit by bit (tests/test_kernel_bodies_cpu.py) and the full-size
    cases take a fifth of the time. The reference order stays sequential."""
    from helpers import usable_cores
    ocore.lib().oracle_set_threads(usable_cores())
    yield
    ocore.lib().oracle_set_threads(1)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMOOTHERS = ('gauss_seidel', 'gauss_seidel_x', 'gauss_seidel_y', 'gauss_seidel_z')


def _case(g, name):
    p = name + '_'
    grid = mg_ref.Grid([g[p + 'hx'], g[p + 'hy'], g[p + 'hz']], g[p + 'origin'])
    ex = np.asfortranarray(g[p + 'eta_x'])
    case = str(g[p + 'case'])
    ey = np.asfortranarray(g[p + 'eta_y']) if case in ('HTI', 'triaxial') else ex
    ez = np.asfortranarray(g[p + 'eta_z']) if case in ('VTI', 'triaxial') else ex
    return grid, mg_ref.VModel(grid, ex, ey, ez, np.asfortranarray(g[p + 'zeta']), case)


def test_library_loaded_and_gpu_visible():
    assert _lib.lib().emg3d_device_count() >= 1
    assert torch.cuda.is_available()


def test_core_smoothers_vs_oracle_four_colour(golden_kernels):
    g = golden_kernels
    for name in g['meta_cases']:
        name = str(name)
        p = name + '_'
        grid, vm = _case(g, name)
        s = mg_ref.Field(grid, g[p + 'gs_s'].copy())
        for fn in SMOOTHERS:
            for nu in (1, 2, 3):
                a = mg_ref.Field(grid, g[p + 'gs_e_in'].copy())
                b = mg_ref.Field(grid, g[p + 'gs_e_in'].copy())
                args = (s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h, nu)
                getattr(ocore, fn)(a.fx, a.fy, a.fz, *args, order=1)
                getattr(core, fn)(b.fx, b.fy, b.fz, *args)
                assert relerr(b.field, a.field) < 2e-12, (name, fn, nu)


def test_core_amat_x_and_restrict_vs_reference_vectors(golden_kernels):
    g = golden_kernels
    for name in g['meta_cases']:
        name = str(name)
        p = name + '_'
        grid, vm = _case(g, name)
        e = mg_ref.Field(grid, g[p + 'amat_e'].copy())
        r = mg_ref.Field(grid, g[p + 'amat_r_in'].copy())
        core.amat_x(r.fx, r.fy, r.fz, e.fx, e.fy, e.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta,
                    *grid.h)
        assert relerr(r.field, g[p + 'amat_r_out']) < 1e-13, name
        res = mg_ref.Field(grid, g[p + 'restrict_res'].copy())
        for sc_dir in range(7):
            q = p + f'sc{sc_dir}_'
            if q + 'csfield' not in g:
                continue
            rx = 1 if sc_dir in (1, 5, 6) else 2
            ry = 1 if sc_dir in (2, 4, 6) else 2
            rz = 1 if sc_dir in (3, 4, 5) else 2
            cgrid = mg_ref.Grid([np.diff(grid.nodes_x[::rx]), np.diff(grid.nodes_y[::ry]),
                                 np.diff(grid.nodes_z[::rz])], grid.origin)
            c = mg_ref.Field(cgrid, dtype=res.field.dtype)
            core.restrict(c.fx, c.fy, c.fz, res.fx, res.fy, res.fz, tuple(g[q + 'wx']),
                          tuple(g[q + 'wy']), tuple(g[q + 'wz']), sc_dir)
            assert relerr(c.field, g[q + 'csfield']) < 1e-14, (name, sc_dir)


def test_core_solve_and_blocks_to_amat_known_answers():
    """The reference's known-answer tests (tests/test_core.py:142-262) through the ABI."""
    amat = np.zeros(90)
    bvec = np.zeros(15)
    mids = [np.array([1, 2, 3, 4, 5, -1, 7, 8, 9, 10, -1, -1, 13, 14, 15, -1, -1, -1, 19, 20,
                      -1, -1, -1, -1, 25], float) + 30 * k for k in range(3)]
    for k in (1, 2):
        mids[k][mids[k] == 30 * k - 1] = -1
    left2 = np.array([6, -1, -1, -1, -1, 11, 12, -1, -1, -1, 16, 17, 18, -1, -1, 21, 22, 23, 24,
                      -1, 26, 27, 28, 29, 30], float)
    left3 = left2 + 30
    left3[left2 == -1] = -1
    core.blocks_to_amat(amat, bvec, mids[0], -np.ones(25), np.arange(1., 6), 0, 3)
    core.blocks_to_amat(amat, bvec, mids[1], left2, np.arange(6., 11), 1, 3)
    core.blocks_to_amat(amat, bvec, mids[2], left3, np.arange(11., 16), 2, 3)
    amat_res = np.arange(1., 91)
    amat_res[5] = amat_res[35] = amat_res[41] = 0
    amat_res[46:48] = 0
    amat_res[51:54] = 0
    amat_res[56:60] = 0
    amat_res[61:] = 0
    bvec_res = np.arange(1., 16)
    bvec_res[11:] = 0
    assert np.array_equal(amat, amat_res) and np.array_equal(bvec, bvec_res)

    rng = np.random.default_rng(3)
    for dtype in (np.float64, np.complex128):
        for n in (6, 21):
            band = np.zeros((n, n), dtype)
            for i in range(n):
                for j in range(max(0, i - 5), i + 1):
                    v = rng.standard_normal() + (1j * rng.standard_normal()
                                                 if dtype == np.complex128 else 0)
                    band[i, j] = band[j, i] = v
            band += 15 * np.eye(n)
            avec = np.zeros(6 * n, dtype)
            for i in range(n):
                for j in range(max(0, i - 5), i + 1):
                    avec[i + 5 * j] = band[i, j]
            x = rng.standard_normal(n).astype(dtype)
            b = band @ x
            a2, b2 = avec.copy(), b.copy()
            core.solve(avec, b)
            ocore.solve(a2, b2)
            assert relerr(b, x) < 1e-12 and relerr(b, b2) < 1e-13 and relerr(avec, a2) < 1e-13


def test_solver_wrappers_vs_reference_vectors(golden_kernels):
    """solver.residual / restriction / prolongation with host objects (reference
    signatures) against vectors produced by the reference's functions of the same name."""
    g = golden_kernels
    for name in g['meta_cases']:
        name = str(name)
        p = name + '_'
        ogrid, vm = _case(g, name)
        grid = emg3d.TensorMesh(ogrid.h, ogrid.origin)
        vm.grid = grid
        freq = float(g[p + 'frequency'])
        e = emg3d.Field(grid, g[p + 'gs_e_in'].copy(), frequency=freq)
        s = emg3d.Field(grid, g[p + 'gs_s'].copy(), frequency=freq)
        assert abs(solver.residual(vm, s, e, True) / g[p + 'residual_norm'] - 1) < 1e-13
        res = emg3d.Field(grid, g[p + 'restrict_res'].copy(), frequency=freq)
        for sc_dir in range(7):
            q = p + f'sc{sc_dir}_'
            if q + 'csfield' not in g:
                continue
            cmodel, cs, ce = solver.restriction(vm, s, res, sc_dir)
            assert relerr(cs.field, g[q + 'csfield']) < 1e-14
            assert np.all(ce.field == 0)
            for k in ('eta_x', 'eta_y', 'eta_z', 'zeta'):
                assert relerr(getattr(cmodel, k), g[q + 'c' + k]) < 1e-15
            assert (cmodel.eta_y is cmodel.eta_x) == (vm.eta_y is vm.eta_x)
            ce = emg3d.Field(cmodel.grid, g[q + 'prol_c'].copy(), frequency=freq)
            fine = emg3d.Field(grid, g[q + 'prol_f_in'].copy(), frequency=freq)
            solver.prolongation(fine, ce, sc_dir)
            assert relerr(fine.field, g[q + 'prol_f_out']) < 1e-14, (name, sc_dir)
            assert relerr(solver._restrict_model_parameters(vm.zeta, sc_dir), g[q + 'czeta']) < 1e-15


def test_smoothing_dispatch(golden_kernels):
    """solver.smoothing == direct kernel calls for lr_dir 0..7 (cf. the reference's
    tests/test_solver.py:380-452), including dropping 2-cell directions."""
    g = golden_kernels
    for name in ('c_tri', 'c_x2', 'c_z2'):
        p = name + '_'
        ogrid, vm = _case(g, name)
        grid = emg3d.TensorMesh(ogrid.h, ogrid.origin)
        vm.grid = grid
        s = emg3d.Field(grid, g[p + 'gs_s'].copy())
        inp = (s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h, 2)
        for lr_dir in range(8):
            a = emg3d.Field(grid, g[p + 'gs_e_in'].copy())
            b = emg3d.Field(grid, g[p + 'gs_e_in'].copy())
            solver.smoothing(vm, s, a, 2, lr_dir)
            c = solver._current_lr_dir(lr_dir, grid)
            if c == 0:
                core.gauss_seidel(b.fx, b.fy, b.fz, *inp)
            if c in (1, 5, 6, 7):
                core.gauss_seidel_x(b.fx, b.fy, b.fz, *inp)
            if c in (2, 4, 6, 7):
                core.gauss_seidel_y(b.fx, b.fy, b.fz, *inp)
            if c in (3, 4, 5, 7):
                core.gauss_seidel_z(b.fx, b.fy, b.fz, *inp)
            assert np.array_equal(a.field, b.field), (name, lr_dir)


def _model_from(g, p, grid):
    kw = {k: g[p + 'res_' + k[-1]] for k in ('property_x', 'property_y', 'property_z')
          if p + 'res_' + k[-1] in g}
    return emg3d.Model(grid, **kw)


@pytest.mark.parametrize('name', ['uni16_F', 'marine16_W', 'tri12x8x16_F', 'lap8_V'])
def test_solve_vs_converged_reference_solves(golden_solves, name):
    """Converged fields within 1e-8 rel-L2 of the reference (both sides tol = 1e-10)."""
    g = golden_solves
    p = name + '_'
    grid = emg3d.TensorMesh([g[p + 'hx'], g[p + 'hy'], g[p + 'hz']], g[p + 'origin'])
    model = _model_from(g, p, grid)
    sfield = emg3d.get_source_field(grid, g[p + 'source'], float(g[p + 'frequency']))
    kw = {k[len(p) + 3:]: g[k].item() for k in g.files if k.startswith(p + 'kw_')}
    efield, info = emg3d.solve(model, sfield, sslsolver=False, return_info=True, **kw)
    assert info['exit'] == 0 and info['exit_message'] == 'CONVERGED'
    assert relerr(efield.field, g[p + 'efield']) < 1e-8
    # a different valid ordering may need a cycle more or less, not many
    assert abs(info["it_mg"] - int(g[p + "it_mg"])) <= 3
    assert info['error_at_cycle'][0] == pytest.approx(float(g[p + 'ref_error']), rel=1e-12)


def test_solve_vs_reference_regression_file(golden_regression):
    """The reference's golden file (tests/test_solver.py:18-60, 152-199, 227-253). The file
    holds fields converged to tol = 1e-6 only, so two valid iteration paths agree to a
    fraction of that, not to 1e-8."""
    g = golden_regression
    for key, cycles in (('res', 'FWV'), ('lap', 'F')):
        grid = emg3d.TensorMesh([g[f'{key}_hx'], g[f'{key}_hy'], g[f'{key}_hz']],
                                g[f'{key}_origin'])
        rho = g[f'{key}_res_xyz']
        model = emg3d.Model(grid, property_x=rho[0], property_y=rho[1], property_z=rho[2])
        sfield = emg3d.get_source_field(grid, g[f'{key}_source'], float(g[f'{key}_frequency']))
        assert relerr(sfield.field, g[f'{key}_sfield']) < 1e-9     # old mu_0 in the file
        for c in cycles:
            e, info = emg3d.solve(model, sfield, plain=True, cycle=c, return_info=True)
            assert info['exit'] == 0
            assert relerr(e.field, g[f'{key}_{c}result']) < 2e-6
            # tightening our tolerance must move us closer to the exact solution both share
            e10 = emg3d.solve(model, sfield, plain=True, cycle=c, tol=1e-11)
            assert relerr(e10.field, g[f'{key}_{c}result']) < 2e-6
    grid = emg3d.TensorMesh([g['reg2_hx'], g['reg2_hy'], g['reg2_hz']], g['reg2_origin'])
    model = emg3d.Model(grid, g['reg2_res_x'], g['reg2_res_y'], g['reg2_res_z'])
    sfield = emg3d.Field(grid, g['reg2_sfield'].copy(), frequency=float(g['reg2_frequency']))
    e, info = emg3d.solve(model, sfield, sslsolver=False, semicoarsening=123, linerelaxation=456,
                          tol=1e-4, maxit=4, nu_init=2, nu_pre=2, nu_coarse=1, nu_post=2,
                          clevel=10, return_info=True)
    assert relerr(e.field, g['reg2_result']) < 5e-4      # both stopped at tol = 1e-4


def test_solve_32_vs_oracle_lexicographic():
    """Config-1 family at 32^3 (docs/dev/tests.rst:193-219) and a stretched VTI case with
    semicoarsening + line relaxation: GPU (4-colour) vs oracle (lexicographic, the
    reference's order), both to tol 1e-10 -> fields within 1e-8."""
    h = np.ones(32) * 50.
    grid = emg3d.TensorMesh([h, h, h], origin=(-800, -800, -800))
    model = emg3d.Model(grid, property_x=1.)
    sfield = emg3d.get_source_field(grid, (0, 0, 0, 0, 0), 1.0)
    e, info = emg3d.solve(model, sfield, plain=True, tol=1e-10, return_info=True)
    assert info['exit'] == 0
    ogrid = mg_ref.Grid(grid.h, grid.origin)
    vm = mg_ref.volume_model(ogrid, 1.0, 1.0)
    eo, io = mg_ref.solve(vm, mg_ref.Field(ogrid, sfield.field.copy()), cycle='F', tol=1e-10)
    assert io['exit'] == 0
    assert relerr(e.field, eo.field) < 1e-8
    assert abs(info["it_mg"] - io["it_mg"]) <= 3

    hx = widths(16, 8, 50, 1.2)
    hz = widths(16, 8, 25, 1.25)
    grid = emg3d.TensorMesh([hx, hx, hz], (-hx.sum() / 2, -hx.sum() / 2, -hz[:20].sum()))
    zc = np.broadcast_to(grid.cell_centers_z[None, None, :], grid.shape_cells)
    rh = np.where(zc > -300, 0.3, 1.0)
    rv = np.where(zc > -300, 0.3, 2.0)
    model = emg3d.Model(grid, property_x=rh, property_z=rv)
    sfield = emg3d.get_source_field(grid, (0, 0, -250, 0, 0), 1.0)
    e, info = emg3d.solve(model, sfield, sslsolver=False, cycle='F', tol=1e-10, return_info=True)
    assert info['exit'] == 0
    ogrid = mg_ref.Grid(grid.h, grid.origin)
    vm = mg_ref.volume_model(ogrid, 1.0, 1 / rh, None, 1 / rv)
    eo, io = mg_ref.solve(vm, mg_ref.Field(ogrid, sfield.field.copy()), cycle='F', tol=1e-10,
                          semicoarsening=True, linerelaxation=True)
    assert io['exit'] == 0
    assert relerr(e.field, eo.field) < 1e-8


def test_solve_conventions_and_edge_cases():
    """Return conventions, warm start, early-outs and failure messages
    (emg3d/solver.py:288-449, 1591-1664; tests/test_solver.py:60-150)."""
    h = widths(4, 2, 30, 1.3)
    grid = emg3d.TensorMesh([h, h, h], (-h.sum() / 2,) * 3)
    model = emg3d.Model(grid, 1.5, 2.0, 3.3)
    sfield = emg3d.get_source_field(grid, (0, 0, 0, 30, 10), 1.0)
    efield = emg3d.solve(model, sfield, plain=True)
    assert isinstance(efield, emg3d.Field)
    # maxit
    _, info = emg3d.solve(model, sfield, plain=True, maxit=2, return_info=True)
    assert info['it_mg'] == 2 and info['exit'] == 1 and 'MAX. ITERATION' in info['exit_message']
    for k in ('exit', 'exit_message', 'abs_error', 'rel_error', 'ref_error', 'tol', 'it_mg',
              'it_ssl', 'time', 'runtime_at_cycle', 'error_at_cycle', 'log'):
        assert k in info
    assert info['error_at_cycle'].size == 3 and info['runtime_at_cycle'].size == 3
    # provided (converged) efield: nothing returned, field unchanged, zero iterations
    ecopy = efield.copy()
    assert emg3d.solve(model, sfield, plain=True, efield=ecopy) is None
    assert np.array_equal(ecopy.field, efield.field)
    info = emg3d.solve(model, sfield, plain=True, efield=ecopy, return_info=True)
    assert info['it_mg'] == 0 and info['exit'] == 0 and info['exit_message'] == 'CONVERGED'
    # warm start from a perturbed field with non-zero boundary values: PEC is enforced
    warm = efield.copy()
    warm.field[:] *= 1.01
    warm.fx[:, 0, :] = 1.0
    emg3d.solve(model, sfield, plain=True, efield=warm)
    assert np.all(warm.fx[:, 0, :] == 0) and relerr(warm.field, efield.field) < 1e-5
    # dtype mismatch, missing frequency
    with pytest.raises(ValueError, match="same dtype"):
        emg3d.solve(model, sfield, plain=True, efield=emg3d.Field(grid, dtype=np.float64))
    wrong = emg3d.Field(grid)
    wrong.field = sfield.field
    with pytest.raises(ValueError, match="missing frequ"):
        emg3d.solve(model, wrong, plain=True)
    # zero source -> zero field; tiny source -> stagnation
    zero = emg3d.Field(grid, frequency=1.0)
    out, info = emg3d.solve(model, zero, plain=True, return_info=True)
    assert np.linalg.norm(out.field) == 0 and info['exit'] == 0
    tiny = emg3d.Field(grid, frequency=1.0)
    tiny.field = 1e-10
    _, info = emg3d.solve(model, tiny, plain=True, maxit=100, return_info=True)
    assert info['exit_message'] in ('STAGNATED', 'CONVERGED')
    # non-finite model -> residual norm is not finite -> DIVERGED (errors surface via the norm)
    bad = emg3d.Model(grid, 1.0)
    bad.property_x[2, 2, 2] = np.inf
    bad.property_x[3, 3, 3] = 0.0
    _, info = emg3d.solve(bad, sfield, plain=True, return_info=True)
    assert info['exit'] == 1
    # verbosity / log capture, exact format of the per-cycle line
    _, info = emg3d.solve(model, sfield, plain=True, verb=4, log=-1, return_info=True)
    assert ' emg3d START ::' in info['log'] and ' MG cycles ' in info['log']
    assert ' CONVERGED' in info['log'] and 'F-cycles   [' in info['log']


def test_krylov_with_multigrid_preconditioner(golden_regression):
    """Default path of emg3d.solve: BiCGSTAB preconditioned by one F-cycle
    (emg3d/solver.py:652-784); against the reference's stored `bicresult`."""
    g = golden_regression
    grid = emg3d.TensorMesh([g['res_hx'], g['res_hy'], g['res_hz']], g['res_origin'])
    rho = g['res_res_xyz']
    model = emg3d.Model(grid, property_x=rho[0], property_y=rho[1], property_z=rho[2])
    sfield = emg3d.get_source_field(grid, g['res_source'], float(g['res_frequency']))
    e, info = emg3d.solve(model, sfield, sslsolver='bicgstab', plain=True, return_info=True)
    assert info['exit'] == 0 and info['it_ssl'] > 0 and info['it_mg'] > 0
    assert relerr(e.field, g['res_bicresult']) < 2e-6
    # the other two solvers of the reference (cgs, gcrotmk), on the device as well
    ec, ic = emg3d.solve(model, sfield, sslsolver='cgs', plain=True, return_info=True)
    assert ic['exit'] == 0 and relerr(ec.field, g['res_bicresult']) < 5e-6
    # gcrotmk: as in the reference's test (tests/test_solver.py:96-98) only that it runs --
    # its preconditioner calls see vectors far from the source's norm, which the reference's
    # own divergence rule (emg3d/solver.py:1627) may abort
    _, ig = emg3d.solve(model, sfield, sslsolver='gcrotmk', plain=True, maxit=1, return_info=True)
    assert ig['exit'] in (0, 1)
    # Krylov alone (no multigrid) and iteration limit
    _, info = emg3d.solve(model, sfield, sslsolver='bicgstab', cycle=None, maxit=3, return_info=True)
    assert info['exit'] == 1 and info['it_ssl'] == 3 and info['it_mg'] == 0
    e2 = emg3d.solve(model, sfield, tol=1e-9)          # all defaults: bicgstab + sc + lr
    e3 = emg3d.solve(model, sfield, sslsolver=False, tol=1e-10)
    assert relerr(e2.field, e3.field) < 1e-7


def _rand_level(shape, case, seed, dtype=torch.complex128, stretch=1.03):
    """Device level with a random model/fields at full size, for property tests."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    h = [widths(n // 2, n // 4, 25., stretch) for n in shape]
    grid = emg3d.TensorMesh(h, (0, 0, 0))
    assert grid.shape_cells == shape
    vol = grid.cell_volumes.reshape(shape, order='F')
    smu0 = 2j * np.pi * 1.0 * 1.25663706127e-06

    class VM:
        pass
    vm = VM()
    vm.grid, vm.case = grid, case
    sig = 10 ** rng.uniform(-1.5, 0.5, shape)
    vm.eta_x = np.asfortranarray(-smu0 * vol * sig)
    vm.eta_y = np.asfortranarray(vm.eta_x / 1.5) if case == 'triaxial' else vm.eta_x
    vm.eta_z = np.asfortranarray(vm.eta_x / 2.5) if case in ('VTI', 'triaxial') else vm.eta_x
    vm.zeta = np.asfortranarray(vol)
    lv = DeviceLevel.from_host(vm, torch.device('cuda'))
    return lv, grid, rng


def _rand_field(lv, grid, seed, pec=True):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    re = torch.randn(grid.n_edges, generator=gen, device='cuda', dtype=torch.float64)
    im = torch.randn(grid.n_edges, generator=gen, device='cuda', dtype=torch.float64)
    t = torch.complex(re, im)
    if pec:
        save = lv.e.clone()
        lv.e.copy_(t)
        lv.pec_zero()
        t = lv.e.clone()
        lv.e.copy_(save)
    return t


@pytest.mark.parametrize('shape,case', [((128, 128, 128), 'VTI'), ((256, 256, 256), 'triaxial')])
def test_full_size_operator_properties(shape, case):
    """BASELINE.json configs 2/3 sizes: A is linear and complex symmetric (x^T A y = y^T A x,
    the property the LDL^T solver relies on, emg3d/core.py:1498-1510); residual(0) = s."""
    lv, grid, _ = _rand_level(shape, case, 1)
    x, y = _rand_field(lv, grid, 2), _rand_field(lv, grid, 3)
    lv.s.zero_()

    def A(v):
        lv.e.copy_(v)
        lv.residual(store=True, norm=False)
        return -lv.r.clone()
    ax, ay = A(x), A(y)
    a, b = 0.7 - 0.2j, -1.3 + 0.5j
    lin = A(a * x + b * y)
    assert (torch.linalg.norm(lin - (a * ax + b * ay)) / torch.linalg.norm(lin)).item() < 1e-13
    xay, yax = torch.sum(x * ay).item(), torch.sum(y * ax).item()
    assert abs(xay - yax) / abs(xay) < 1e-11
    lv.s.copy_(x)
    lv.e.zero_()
    n = lv.residual(store=True, norm=True)
    assert torch.equal(lv.r, x)
    assert n == pytest.approx(torch.linalg.norm(x).item(), rel=1e-13)


@pytest.mark.parametrize('shape,case', [((128, 128, 128), 'VTI'), ((256, 256, 256), 'triaxial')])
def test_full_size_smoother_fixed_point_and_reduction(shape, case):
    """If s = A e* then every smoother leaves e* unchanged (idempotence at the solution);
    from e = 0 each sweep must reduce the residual. Line smoothers solve their lines
    exactly, so after one x-line sweep the residual on ... is checked through the norm."""
    lv, grid, _ = _rand_level(shape, case, 4)
    estar = _rand_field(lv, grid, 5)
    lv.s.zero_()
    lv.e.copy_(estar)
    lv.residual(store=True, norm=False)
    lv.s.copy_(-lv.r)                       # s = A e*
    enorm = torch.linalg.norm(estar).item()
    for lr in (0, 1, 2, 3):
        lv.e.copy_(estar)
        lv.smooth(lr, 2)
        assert (torch.linalg.norm(lv.e - estar).item() / enorm) < 1e-9, lr
    lv.e.zero_()
    r0 = lv.residual(store=False, norm=True)
    for lr in (0, 1, 2, 3):
        lv.e.zero_()
        lv.smooth(lr, 1)
        r1 = lv.residual(store=False, norm=True)
        assert np.isfinite(r1) and r1 < r0, (lr, r1, r0)


def test_tuning_options_do_not_change_results(golden_kernels):
    """emg3d_set_option knobs (launch schedules) must be result-neutral on the GPU too."""
    lib = _lib.lib()
    g = golden_kernels
    p = 'c_tri_'
    grid, vm = _case(g, 'c_tri')
    s = mg_ref.Field(grid, g[p + 'gs_s'].copy())
    args = (s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h, 2)
    ref = {}
    try:
        for fn in SMOOTHERS:
            a = mg_ref.Field(grid, g[p + 'gs_e_in'].copy())
            lib.emg3d_set_option(b'point_slab', 0)
            lib.emg3d_set_option(b'line_fuse', 0)
            getattr(core, fn)(a.fx, a.fy, a.fz, *args)
            ref[fn] = a.field.copy()
        for slab, fuse, lds in ((2, 1, 1), (3, 2, 0), (5, 1, 0), (0, 2, 1)):
            lib.emg3d_set_option(b'point_slab', slab)
            lib.emg3d_set_option(b'line_fuse', fuse)
            lib.emg3d_set_option(b'line_lds', lds)
            for fn in SMOOTHERS:
                b = mg_ref.Field(grid, g[p + 'gs_e_in'].copy())
                getattr(core, fn)(b.fx, b.fy, b.fz, *args)
                assert np.array_equal(b.field, ref[fn]), (fn, slab, fuse, lds)
    finally:
        lib.emg3d_set_option(b'point_slab', 0)
        lib.emg3d_set_option(b'line_fuse', 2)
        lib.emg3d_set_option(b'line_lds', 1)


@pytest.mark.parametrize('tile_min', [0, 1])
def test_point_order_option_vs_oracle(tile_min):
    """Option point_order: 1 (default) = every sweep of the point smoother visits the node colours in the same
    sequence 0,2,3,1; 0 = backward sweeps mirrored (rounds 1-2). Both against the oracle in the same order, plain
    and tiled schedule, nu = 3 (2e-12); and a plain-multigrid solve must not need more cycles with the default."""
    lib, olib = _lib.lib(), ocore.lib()
    rng = np.random.default_rng(78)
    shape = (40, 14, 18)
    h = [rng.uniform(5., 15., n) * 1.05 ** np.abs(np.arange(n) - n // 2) for n in shape]
    grid = mg_ref.Grid(h, (0., 0., 0.))
    sig = [10 ** rng.uniform(-1, 1, shape) for _ in range(3)]
    vm = mg_ref.volume_model(grid, 0.9, *sig)
    s, e0 = mg_ref.Field(grid), mg_ref.Field(grid)
    for f in (s, e0):
        f.field[:] = rng.standard_normal(f.field.size) + 1j * rng.standard_normal(f.field.size)
    for f in (e0.fx[:, 0, :], e0.fx[:, -1, :], e0.fx[:, :, 0], e0.fx[:, :, -1], e0.fy[0], e0.fy[-1],
              e0.fy[:, :, 0], e0.fy[:, :, -1], e0.fz[0], e0.fz[-1], e0.fz[:, 0], e0.fz[:, -1]):
        f[...] = 0
    args = (s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h, 3)
    hx = widths(12, 6, 40., 1.15)
    g2 = emg3d.TensorMesh([hx, hx, hx], (-hx.sum() / 2,) * 3)
    model = emg3d.Model(g2, 10 ** np.random.default_rng(3).uniform(-0.3, 0.7, g2.shape_cells))
    sf = emg3d.get_source_field(g2, (0., 0., 0., 10., 20.), 1.0)
    old_tile = lib.emg3d_get_option(b'point_tile_min')
    out, cycles = {}, {}
    try:
        lib.emg3d_set_option(b'point_tile_min', tile_min)
        for order in (0, 1):
            lib.emg3d_set_option(b'point_order', order)
            olib.oracle_set_point_repeat(order)
            a, b = e0.copy(), e0.copy()
            ocore.gauss_seidel(a.fx, a.fy, a.fz, *args, order=2 if tile_min else 1)
            core.gauss_seidel(b.fx, b.fy, b.fz, *args)
            assert relerr(b.field, a.field) < 2e-12, order
            out[order] = b.field.copy()
            _, info = emg3d.solve(model, sf, sslsolver=False, plain=True, cycle='F', tol=1e-8, return_info=True)
            assert info['exit'] == 0
            cycles[order] = info['it_mg']
    finally:
        lib.emg3d_set_option(b'point_tile_min', old_tile)
        lib.emg3d_set_option(b'point_order', 1)
        olib.oracle_set_point_repeat(1)
    assert relerr(out[0], out[1]) > 1e-6
    assert cycles[1] <= cycles[0], cycles


def test_line_order_option_mirrored_and_cyclic_vs_oracle():
    """Option line_order: 1 (default) = the colour passes of a line-smoothing call cycle through 1,2,3,0,1,...;
    0 = mirrored sweeps (rounds 1-2); 2 = the same sequence 1,2,3,0 in every sweep (4 nu launches, no shared pass).
    Each against the oracle in the same order, per call (nu = 3, 2e-12), and on the reduced copy of config 3 the
    cyclic order must not need more cycles than the mirrored one (oracle: 21 against 24 at tol 1e-10), the
    repeated one not more than the cyclic one."""
    from bench import workload
    lib, olib = _lib.lib(), ocore.lib()
    rng = np.random.default_rng(77)
    shape = (20, 14, 18)
    h = [rng.uniform(5., 15., n) * 1.05 ** np.abs(np.arange(n) - n // 2) for n in shape]
    grid = mg_ref.Grid(h, (0., 0., 0.))
    sig = [10 ** rng.uniform(-1, 1, shape) for _ in range(3)]
    vm = mg_ref.volume_model(grid, 0.9, *sig)
    s, e0 = mg_ref.Field(grid), mg_ref.Field(grid)
    for f in (s, e0):
        f.field[:] = rng.standard_normal(f.field.size) + 1j * rng.standard_normal(f.field.size)
    for f in (e0.fx[:, 0, :], e0.fx[:, -1, :], e0.fx[:, :, 0], e0.fx[:, :, -1], e0.fy[0], e0.fy[-1],
              e0.fy[:, :, 0], e0.fy[:, :, -1], e0.fz[0], e0.fz[-1], e0.fz[:, 0], e0.fz[:, -1]):
        f[...] = 0
    args = (s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h, 3)
    ws = workload('triaxial64')
    g64 = emg3d.TensorMesh(ws['h'], ws['origin'])
    model = emg3d.Model(g64, **ws['res'])
    sf = emg3d.get_source_field(g64, ws['source'], ws['frequency'])
    cycles, fields = {}, {}
    try:
        for order in (0, 1, 2):
            lib.emg3d_set_option(b'line_order', order)
            olib.oracle_set_line_order(order, 1, 2, 3, 0)
            for fn in SMOOTHERS[1:]:
                a, b = e0.copy(), e0.copy()
                getattr(ocore, fn)(a.fx, a.fy, a.fz, *args, order=1)
                getattr(core, fn)(b.fx, b.fy, b.fz, *args)
                assert relerr(b.field, a.field) < 2e-12, (order, fn)
                fields[(order, fn)] = b.field.copy()
            e, info = emg3d.solve(model, sf, sslsolver=False, tol=1e-8, return_info=True, **ws['opts'])
            assert info['exit'] == 0
            cycles[order], fields[order] = info['it_mg'], e.field.copy()
    finally:
        lib.emg3d_set_option(b'line_order', 1)
        olib.oracle_set_line_order(1, 1, 2, 3, 0)
    assert all(relerr(fields[(0, fn)], fields[(1, fn)]) > 1e-6 for fn in SMOOTHERS[1:])     # the orders do differ
    assert relerr(fields[1], fields[0]) < 1e-7                                               # ... the solutions do not
    assert all(relerr(fields[(2, fn)], fields[(1, fn)]) > 1e-6 for fn in SMOOTHERS[1:])
    assert relerr(fields[2], fields[0]) < 1e-7
    assert cycles[1] <= cycles[0] - 1 and cycles[2] <= cycles[1], cycles


@pytest.mark.parametrize('shape,lr', [((64, 96, 96), 1), ((96, 64, 96), 2), ((96, 96, 130), 3), ((258, 96, 96), 1),
                                      ((60, 384, 60), 2)])
@pytest.mark.parametrize('dtype', [complex, float])
def test_streamed_line_kernel_is_bit_identical(shape, lr, dtype):
    """k_line_stream (right-hand sides produced into an LDS ring while the forward chains run) against
    k_line_colour (line_stream = 0): the same arithmetic entry by entry, so the fields after nu = 3 sweeps
    must agree bit for bit. Shapes: 64-block lines whose records fit in LDS (k_line_colour either way),
    130-block lines (records partly in LDS before), 258-block lines (global scratch), each with enough
    lines per colour class for 16-line workgroups; and 384-block lines with 8 lines per workgroup (half-
    filled chain waves, surplus quads)."""
    lib = _lib.lib()
    rng = np.random.default_rng(sum(shape) + lr)
    h = [rng.uniform(5., 15., n) * 1.02 ** np.abs(np.arange(n) - n // 2) for n in shape]
    grid = mg_ref.Grid(h, (0., 0., 0.))
    sig = [10 ** rng.uniform(-1, 1, shape) for _ in range(3)]
    vm = mg_ref.volume_model(grid, 0.7 if dtype is complex else -0.7, *sig)
    s, e0 = mg_ref.Field(grid, dtype=dtype), mg_ref.Field(grid, dtype=dtype)
    for f in (s, e0):
        f.field[:] = rng.standard_normal(f.field.size)
        if dtype is complex:
            f.field[:] += 1j * rng.standard_normal(f.field.size)
    for f in (e0.fx[:, 0, :], e0.fx[:, -1, :], e0.fx[:, :, 0], e0.fx[:, :, -1], e0.fy[0], e0.fy[-1],
              e0.fy[:, :, 0], e0.fy[:, :, -1], e0.fz[0], e0.fz[-1], e0.fz[:, 0], e0.fz[:, -1]):
        f[...] = 0
    args = (s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h, 3)
    out = {}
    old = lib.emg3d_get_option(b'line_stream')
    try:
        for mode in (0, 2):          # 2: streamed also where part of the records would fit in LDS (130-block lines)
            lib.emg3d_set_option(b'line_stream', mode)
            b = e0.copy()
            getattr(core, SMOOTHERS[lr])(b.fx, b.fy, b.fz, *args)
            out[mode] = b.field.copy()
    finally:
        lib.emg3d_set_option(b'line_stream', old)
    assert np.any(out[0] != e0.field)
    assert np.array_equal(out[2], out[0])


SHORT_SHAPES = [((2, 37, 11), 1), ((3, 36, 12), 1), ((4, 150, 5), 1), ((5, 33, 9), 1), ((6, 40, 40), 1),
                ((8, 70, 9), 1), ((9, 34, 35), 1), ((10, 20, 90), 1), ((130, 4, 4), 2), ((70, 5, 8), 2),
                ((41, 6, 4), 2), ((35, 8, 37), 2), ((12, 10, 300), 2), ((256, 4, 4), 3), ((9, 70, 3), 3),
                ((20, 21, 6), 3), ((66, 8, 8), 3), ((8, 8, 9), 3), ((5, 4, 10), 3),
                ((7, 30, 31), 1), ((11, 40, 9), 1), ((16, 33, 34), 1), ((33, 70, 6), 1), ((64, 40, 40), 1),
                ((50, 12, 9), 2), ((9, 24, 70), 2), ((40, 63, 40), 2), ((30, 31, 17), 3), ((70, 5, 32), 3),
                ((36, 36, 66), 3)]


@pytest.mark.parametrize('shape,lr', SHORT_SHAPES)
@pytest.mark.parametrize('dtype', [complex, float])
def test_short_lines_vs_oracle(shape, lr, dtype):
    """Every short line length (2, 3, 4, 5, 6 blocks: padding granule 2; 7 ... 11: halves of one register ring or
    none, with and without identity padding) and lines of 12 ... 66 blocks whose records live in LDS, on rod-, slab-
    and cube-shaped levels (1 ... 400 lines per colour class, workgroups of 4, 8 and 16 lines, surplus quads):
    nu = 3 sweeps against the oracle in the same ordering."""
    grid, vm, s0, e0 = _random_level_fields(shape, dtype, sum(shape) + 7 * lr)
    a, b = e0.copy(), e0.copy()
    args = (s0.fx, s0.fy, s0.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h, 3)
    getattr(ocore, SMOOTHERS[lr])(a.fx, a.fy, a.fz, *args, order=1)
    getattr(core, SMOOTHERS[lr])(b.fx, b.fy, b.fz, *args)
    assert np.any(b.field != e0.field)
    assert relerr(b.field, a.field) < 1e-11


def _random_long_line_level(shape, lr, dtype):
    rng = np.random.default_rng(sum(shape) + lr)
    h = [rng.uniform(5., 15., n) * 1.02 ** np.abs(np.arange(n) - n // 2) for n in shape]
    grid = mg_ref.Grid(h, (0., 0., 0.))
    sig = [10 ** rng.uniform(-1, 1, shape) for _ in range(3)]
    vm = mg_ref.volume_model(grid, 0.7 if dtype is complex else -0.7, *sig)
    s, e0 = mg_ref.Field(grid, dtype=dtype), mg_ref.Field(grid, dtype=dtype)
    for f in (s, e0):
        f.field[:] = rng.standard_normal(f.field.size)
        if dtype is complex:
            f.field[:] += 1j * rng.standard_normal(f.field.size)
    for f in (e0.fx[:, 0, :], e0.fx[:, -1, :], e0.fx[:, :, 0], e0.fx[:, :, -1], e0.fy[0], e0.fy[-1],
              e0.fy[:, :, 0], e0.fy[:, :, -1], e0.fz[0], e0.fz[-1], e0.fz[:, 0], e0.fz[:, -1]):
        f[...] = 0
    return grid, vm, s, e0


@pytest.mark.parametrize('shape,lr,lpw', [((258, 96, 96), 1, 0), ((96, 130, 96), 2, 0), ((24, 20, 257), 3, 16), ((130, 9, 30), 1, 16),
                                          ((20, 384, 22), 2, 16), ((40, 40, 260), 3, 16)])
@pytest.mark.parametrize('dtype', [complex, float])
def test_compact_streamed_line_kernel_vs_cpu_walk(shape, lr, lpw, dtype):
    """COMPACT line records (k_line_stream<.., COMPACT>; emg3d_level flag LINE_COMPACT): the inverse blocks T_k and the
    forward pass's w records stored in SINGLE precision, every operation in fp64. Per sweep (nu = 3) against the CPU
    walk of the same solve with the same two roundings (tests/emu: stencil.h line_forward_ref / line_backward_ref with
    FT = WT = compact_of<T>), run on the very T records the HIP set-up kernel stored (copied back from HBM): what is left
    between the two are the w values that lie within the fp64 differences of the two evaluations (1e-13) of a
    single-precision rounding boundary -- a few in a million, each worth one ordinary rounding error. And against the
    CPU walk's own compact set-up (the same T up to such flips) and the fp64 records (different: the storage is
    really narrower; close: eps32 x cond of the blocks). 130 ... 384-block lines in all three directions, 16-line
    workgroups forced on levels with few lines (surplus quads, part-filled workgroups), real and complex."""
    from emu import emu
    lib = _lib.lib()
    grid, vm, s, e0 = _random_long_line_level(shape, lr, dtype)
    dev = torch.device('cuda')
    out = {}
    with _option('line_lpw', lpw):
        if lib.emg3d_line_kernel_name(lr, *shape, int(dtype is complex), 1) != b'k_line_stream':
            pytest.skip('the records of these lines fit in LDS: k_line_colour, no compact form')
        for compact in (0, 1):
            lv = DeviceLevel.from_host(vm, dev)
            if compact:
                lv.set_line_compact(True)
            assert lib.emg3d_line_compact_used(lv._cref, lr) == compact
            lv.s.copy_(torch.from_numpy(s.field))
            lv.e.copy_(torch.from_numpy(e0.field))
            lv.smooth(lr, 3)
            out[compact] = lv.e.cpu().numpy()
            fac, lfac = (t.cpu().numpy() for t in lv.line_factors(lr))
        assert fac.size * 2 == lib.emg3d_line_fac_bytes(lr, *shape, int(dtype is complex))     # half the bytes
    emu.lib().emu_set_line_compact(1)
    try:
        ref, ref2 = e0.copy(), e0.copy()
        emu.gauss_seidel_fac(ref, s, vm, lr, 3, fac, lfac.view(np.float64))
        emu.gauss_seidel(ref2, s, vm, lr, 3)
    finally:
        emu.lib().emu_set_line_compact(0)
    assert np.any(out[1] != e0.field)
    d = relerr(out[1], out[0])                 # what the narrower storage changes: ~ eps32 x cond of the blocks
    dc = relerr(out[1], ref.field)             # kernel against the CPU walk on the kernel's own T records
    ds = relerr(out[1], ref2.field)            # ... on the CPU set-up's (rounding flips of T entries included)
    print(f"compact {shape} lr={lr} {dtype.__name__}: vs fp64 records {d:.2e}, vs CPU walk (same T) {dc:.2e}, (own T) {ds:.2e}")
    assert 1e-9 < d < 3e-2, d
    # (measured: 5e-14 ... 1e-9 on the levels with few lines, 0.5 ... 4 % of d on those with millions of values)
    assert dc < 0.1 * d, (dc, d)


@pytest.mark.parametrize('shape,lr,opts', [((64, 40, 40), 1, {}), ((40, 63, 40), 2, {}), ((36, 36, 66), 3, {}), ((100, 70, 70), 1, {}),
                                           ((20, 128, 30), 2, {'line_lpw': 16, 'line_stream': 1}), ((12, 10, 300), 3, {})])
@pytest.mark.parametrize('dtype', [complex, float])
def test_compact_three_phase_line_kernel_vs_cpu_walk(shape, lr, opts, dtype):
    """COMPACT T records on the levels that run k_line_colour (lines of 7 ... ~128 blocks whose right-hand-side /
    solution records live in LDS -- those stay fp64): per sweep against the CPU walk with single-precision T records and
    fp64 w records on the kernel's own T records (tests/emu, g_line_compact = 2). Records in LDS (mode 1), slots 0..3 in
    LDS (mode 2, option line_stream = 1), 4- and 8- and 16-line workgroups."""
    from emu import emu
    from contextlib import ExitStack
    lib = _lib.lib()
    grid, vm, s, e0 = _random_long_line_level(shape, lr, dtype)
    dev = torch.device('cuda')
    out = {}
    with ExitStack() as stack:
        for k, v in opts.items():
            stack.enter_context(_option(k, v))
        if lib.emg3d_line_kernel_name(lr, *shape, int(dtype is complex), 1) != b'k_line_colour':
            pytest.skip('not a k_line_colour level for this dtype')
        for compact in (0, 1):
            lv = DeviceLevel.from_host(vm, dev)
            if compact:
                lv.set_line_compact(True)
                if not lib.emg3d_line_compact_used(lv._cref, lr):
                    # a class with few lines (4- or 8-line workgroups, or slots 0..3 in LDS) runs the STREAMED kernel as soon
                    # as it carries a batch: such a level keeps fp64 records for everybody, so that a source gives the same
                    # bits alone and in a batch (kernels.hip: line_compact_used)
                    assert shape in ((20, 128, 30), (12, 10, 300))
                    pytest.skip('the level streams for batches: fp64 records for single sources too')
            assert lib.emg3d_line_compact_used(lv._cref, lr) == compact
            lv.s.copy_(torch.from_numpy(s.field))
            lv.e.copy_(torch.from_numpy(e0.field))
            lv.smooth(lr, 3)
            out[compact] = lv.e.cpu().numpy()
            fac, lfac = (t.cpu().numpy() for t in lv.line_factors(lr))
    emu.lib().emu_set_line_compact(2)
    try:
        ref = e0.copy()
        emu.gauss_seidel_fac(ref, s, vm, lr, 3, fac, lfac.view(np.float64))
    finally:
        emu.lib().emu_set_line_compact(0)
    d = relerr(out[1], out[0])
    dc = relerr(out[1], ref.field)
    print(f"compact three-phase {shape} lr={lr} {dtype.__name__}: vs fp64 records {d:.2e}, vs CPU walk (same T) {dc:.2e}")
    assert 1e-10 < d < 3e-2, d
    assert dc < 5e-12, dc       # (no rounding of w here: nothing can flip; measured 3e-13 complex, 2e-12 real)


class _option:
    """Set a run-time option of the library for the duration of a with-block."""

    def __init__(self, name, value):
        self.name, self.value = name.encode(), int(value)

    def __enter__(self):
        lib = _lib.lib()
        self.old = lib.emg3d_get_option(self.name)
        assert lib.emg3d_set_option(self.name, self.value) == 0
        return self

    def __exit__(self, *exc):
        _lib.lib().emg3d_set_option(self.name, self.old)


WIDE_SHAPES = [(sh, lr) for sh, lr in SHORT_SHAPES if sh[lr - 1] <= 64]


@pytest.mark.parametrize('shape,lr', WIDE_SHAPES)
@pytest.mark.parametrize('dtype', [complex, float])
def test_wide_line_kernel_vs_oracle(shape, lr, dtype):
    """k_line_wide (option line_wide: four-unknown chains on sixteen lanes per half-line, one thread per block for the
    rest) on every short line length -- 2 ... 64 blocks: no top half, no bottom half, halves of unequal length, one
    to eight lines per workgroup, surplus chain groups -- nu = 3 sweeps against the oracle in the same ordering,
    and against the kernel the level runs otherwise (same factors, N = T C rounded once more: equal to rounding)."""
    grid, vm, s0, e0 = _random_level_fields(shape, dtype, sum(shape) + 7 * lr)
    a, b, c = e0.copy(), e0.copy(), e0.copy()
    args = (s0.fx, s0.fy, s0.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h, 3)
    getattr(ocore, SMOOTHERS[lr])(a.fx, a.fy, a.fz, *args, order=1)
    with _option('line_wide', 0):
        getattr(core, SMOOTHERS[lr])(c.fx, c.fy, c.fz, *args)
    with _option('line_wide', 64):
        assert _lib.lib().emg3d_line_kernel_name(lr, *shape, int(dtype is complex), 1) == b'k_line_wide'
        getattr(core, SMOOTHERS[lr])(b.fx, b.fy, b.fz, *args)
    assert np.any(b.field != e0.field)
    assert relerr(b.field, a.field) < 1e-11
    assert relerr(b.field, c.field) < 1e-11


@pytest.mark.parametrize('shape,lr', [((5, 33, 9), 1), ((35, 8, 37), 2), ((70, 5, 32), 3), ((33, 70, 6), 1), ((40, 63, 40), 2)])
def test_wide_line_kernel_block_thread_count_does_not_change_bits(shape, lr):
    """k_line_wide with 192 and with 256 block threads per workgroup (option line_wide_bt; 0 picks 256 where it gives a
    workgroup more lines, i.e. on lines of 26 and more blocks): another distribution of the same blocks over threads and
    workgroups -- 6 / 8 lines of 32 blocks, the middle blocks in wave 3 / wave 4 -- and the same bits."""
    grid, vm, s0, e0 = _random_level_fields(shape, complex, sum(shape) + 3 * lr)
    args = (s0.fx, s0.fy, s0.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h, 3)
    out = []
    for bt in (0, 192, 256):
        b = e0.copy()
        with _option('line_wide', 64), _option('line_wide_bt', bt):
            getattr(core, SMOOTHERS[lr])(b.fx, b.fy, b.fz, *args)
        out.append(b.field.copy())
    assert np.any(out[0] != e0.field)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


@pytest.mark.parametrize('shape,lr', [((4, 40, 9), 1), ((34, 16, 30), 2), ((20, 21, 64), 3)])
@pytest.mark.parametrize('batch,dtype', [(2, complex), (5, complex), (3, float)])
def test_wide_line_kernel_batch_equals_single_source(shape, lr, batch, dtype):
    """k_line_wide with several right-hand sides (grid.y = right-hand side) gives every source the bits it gets alone."""
    grid, vm, s0, e0 = _random_level_fields(shape, dtype, sum(shape) + lr + batch)
    dev = torch.device('cuda')
    rng = np.random.default_rng(batch)
    n = e0.field.size
    srcs = [s0.field * (1 + b) + (0.3 * b) * rng.standard_normal(n) for b in range(batch)]
    starts = [e0.field * (1.0 - 0.2 * b) for b in range(batch)]
    with _option('line_wide', 64):
        assert _lib.lib().emg3d_line_kernel_name(lr, *shape, int(dtype is complex), batch) == b'k_line_wide'
        single = DeviceLevel.from_host(vm, dev)
        want = []
        for b in range(batch):
            single.s.copy_(torch.from_numpy(srcs[b]))
            single.e.copy_(torch.from_numpy(starts[b]))
            single.smooth(lr, 3)
            want.append(single.e.cpu().numpy())
        many = DeviceLevel.from_host(vm, dev, batch=batch)
        many._factors = single._factors              # the same factor buffers (they depend on the model only)
        many.s.copy_(torch.from_numpy(np.concatenate(srcs)))
        many.e.copy_(torch.from_numpy(np.concatenate(starts)))
        many.smooth(lr, 3)
        got = many.e.cpu().numpy().reshape(batch, n)
    for b in range(batch):
        assert np.any(want[b] != starts[b])
        assert np.array_equal(got[b], want[b]), (b, relerr(got[b], want[b]))


def _random_level_fields(shape, dtype, seed, freq=0.7, extras=False):
    """Stretched random tri-axial model on `shape` (oracle volume model) with random source / start fields
    (PEC faces of the start field zero); extras: with epsilon_r and mu_r (eta gets a real part)."""
    rng = np.random.default_rng(seed)
    h = [rng.uniform(5., 15., n) * 1.02 ** np.abs(np.arange(n) - n // 2) for n in shape]
    grid = mg_ref.Grid(h, (0., 0., 0.))
    sig = [10 ** rng.uniform(-1, 1, shape) for _ in range(3)]
    kw = dict(mu_r=rng.uniform(0.8, 2.0, shape), epsilon_r=rng.uniform(1., 80., shape)) if extras else {}
    vm = mg_ref.volume_model(grid, freq if dtype is complex else -abs(freq), *sig, **kw)
    fields = []
    for _ in range(2):
        f = mg_ref.Field(grid, dtype=dtype)
        f.field[:] = rng.standard_normal(f.field.size)
        if dtype is complex:
            f.field[:] += 1j * rng.standard_normal(f.field.size)
        fields.append(f)
    e0 = fields[1]
    for f in (e0.fx[:, 0, :], e0.fx[:, -1, :], e0.fx[:, :, 0], e0.fx[:, :, -1], e0.fy[0], e0.fy[-1],
              e0.fy[:, :, 0], e0.fy[:, :, -1], e0.fz[0], e0.fz[-1], e0.fz[:, 0], e0.fz[:, -1]):
        f[...] = 0
    return grid, vm, fields[0], e0


@pytest.mark.parametrize('shape,lr', [((130, 72, 72), 1), ((72, 130, 72), 2), ((72, 72, 258), 3), ((384, 66, 66), 1),
                                      ((66, 384, 66), 2)])
@pytest.mark.parametrize('batch,dtype', [(2, complex), (3, complex), (4, complex), (5, complex), (4, float), (8, complex)])
def test_batched_streamed_line_kernel_equals_single_source(shape, lr, batch, dtype):
    """k_line_stream with B > 1 -- one workgroup serves its 16 lines for a group of up to four right-hand sides,
    every factor row fetched once per group -- against the single-source launches on the same level: source by source the fields after nu = 3 sweeps must agree BIT
    FOR BIT (batches of 5 and 8 run as groups of 3 + 2 and 4 + 4). Lines of 130 and 258 blocks (R = 16 / 8
    rows per chunk, several chunks, a ragged last one), > 1000 lines per colour class (16 per workgroup); lines of
    384 blocks -- config 5's own line length (384 x 256 x 256): three ring chunks per half at R = 16 with a ragged
    last one, six at R = 8 -- in groups of two, three and four (x-lines) and as 3 + 2 / 4 + 4 (y-lines)."""
    lib = _lib.lib()
    if batch >= 5 and lr != 2:
        pytest.skip('group splitting is direction-independent: one direction is enough')
    if dtype is float and lr != 3:
        pytest.skip('the records of 16 real 130-block lines fit in LDS: k_line_colour')
    assert lib.emg3d_line_kernel_name(lr, *shape, int(dtype is complex), batch) == b'k_line_stream'
    grid, vm, s0, e0 = _random_level_fields(shape, dtype, sum(shape) + lr + batch)
    dev = torch.device('cuda')
    rng = np.random.default_rng(batch)
    n = e0.field.size
    srcs = [s0.field * (1 + b) + (0.3 * b) * rng.standard_normal(n) for b in range(batch)]
    starts = [e0.field * (1.0 - 0.2 * b) for b in range(batch)]
    single = DeviceLevel.from_host(vm, dev)
    want = []
    for b in range(batch):
        single.s.copy_(torch.from_numpy(srcs[b]))
        single.e.copy_(torch.from_numpy(starts[b]))
        single.smooth(lr, 3)
        want.append(single.e.cpu().numpy())
    many = DeviceLevel.from_host(vm, dev, batch=batch)
    many._factors = single._factors              # the same factor buffers (they depend on the model only)
    many.s.copy_(torch.from_numpy(np.concatenate(srcs)))
    many.e.copy_(torch.from_numpy(np.concatenate(starts)))
    many.smooth(lr, 3)
    got = many.e.cpu().numpy().reshape(batch, n)
    for b in range(batch):
        assert np.any(want[b] != starts[b])
        assert np.array_equal(got[b], want[b]), (b, relerr(got[b], want[b]))


@pytest.mark.parametrize('shape,lr', [((130, 72, 72), 1), ((72, 130, 72), 2), ((72, 72, 258), 3)])
@pytest.mark.parametrize('batch', [2, 3, 4])
def test_batched_compact_line_kernel_equals_single_source(shape, lr, batch):
    """Groups of right-hand sides on a level with COMPACT line records (k_line_stream<.., B, COMPACT>): the group's chain
    quads widen one single-precision factor row and apply it to all of its sources, every source's w records are rounded
    as the single-source kernel rounds them -- source by source BIT FOR BIT the single-source compact result."""
    lib = _lib.lib()
    grid, vm, s0, e0 = _random_level_fields(shape, complex, sum(shape) + lr + batch)
    dev = torch.device('cuda')
    rng = np.random.default_rng(batch)
    n = e0.field.size
    srcs = [s0.field * (1 + b) + (0.3 * b) * rng.standard_normal(n) for b in range(batch)]
    starts = [e0.field * (1.0 - 0.2 * b) for b in range(batch)]
    with _option('line_lpw', 16):     # (16-line workgroups for the single source too: its ~1 250 lines per class would get 8)
        single = DeviceLevel.from_host(vm, dev)
        single.set_line_compact(True)
        assert lib.emg3d_line_compact_used(single._cref, lr) == 1
        want = []
        for b in range(batch):
            single.s.copy_(torch.from_numpy(srcs[b]))
            single.e.copy_(torch.from_numpy(starts[b]))
            single.smooth(lr, 3)
            want.append(single.e.cpu().numpy())
        many = DeviceLevel.from_host(vm, dev, batch=batch)
        many.set_line_compact(True)
        assert lib.emg3d_line_compact_used(many._cref, lr) == 1
        many.s.copy_(torch.from_numpy(np.concatenate(srcs)))
        many.e.copy_(torch.from_numpy(np.concatenate(starts)))
        many.smooth(lr, 3)
        got = many.e.cpu().numpy().reshape(batch, n)
    for b in range(batch):
        assert np.any(want[b] != starts[b])
        assert np.array_equal(got[b], want[b]), (b, relerr(got[b], want[b]))


def test_solve_batch_long_lines_equals_separate_solves():
    """solve_batch on a grid whose finest level runs k_line_stream (lines of 256 blocks along x, 72 x 72
    lines): fields, cycle counts and error histories of four sources bit-identical to separate solves."""
    lib = _lib.lib()
    shape = (256, 72, 72)
    h = [widths(n // 2, n // 4, 30., 1.04) for n in shape]
    grid = emg3d.TensorMesh(h, [-w.sum() / 2 for w in h])
    assert grid.shape_cells == shape
    assert lib.emg3d_line_kernel_name(1, *shape, 1, 4) == b'k_line_stream'
    rng = np.random.default_rng(8)
    rho = 10 ** rng.uniform(-0.5, 0.7, shape)
    model = emg3d.Model(grid, rho, 1.5 * rho, 2.0 * rho)
    sfields = [emg3d.get_source_field(grid, (x, y, 5., az, 0.), 1.0)
               for x, y, az in ((-300., 20., 0.), (100., -60., 45.), (0., 0., 90.), (250., 120., 20.))]
    kw = dict(cycle='F', semicoarsening=True, linerelaxation=True, tol=1e-6)
    sep = [emg3d.solve(model, sf, sslsolver=False, return_info=True, **kw) for sf in sfields]
    bat = emg3d.solve_batch(model, sfields, **kw)
    for (e1, i1), (e2, i2) in zip(sep, bat):
        assert i1['exit'] == i2['exit'] == 0 and i1['it_mg'] == i2['it_mg']
        assert np.array_equal(i1['error_at_cycle'], i2['error_at_cycle'])
        assert np.array_equal(e1.field, e2.field)


@pytest.mark.parametrize('lpw', [32, 16, 8])
def test_line_lpw_option_on_long_lines_vs_default(lpw):
    """Option line_lpw on a level with lines of 96+ blocks (advisor finding of round 3: with 32 lines per
    workgroup the streamed kernel, whose two chain waves serve 16 lines, left lines 16..31 of every
    workgroup unsmoothed): the launcher must keep such launches with k_line_colour, and the fields must not
    depend on the option."""
    lib = _lib.lib()
    shape = (40, 200, 40)
    grid, vm, s, e0 = _random_level_fields(shape, complex, 77)
    args = (s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h, 2)
    out = {}
    old = lib.emg3d_get_option(b'line_lpw')
    try:
        for v in (0, lpw):
            assert lib.emg3d_set_option(b'line_lpw', v) == 0
            b = e0.copy()
            core.gauss_seidel_y(b.fx, b.fy, b.fz, *args)
            out[v] = b.field.copy()
    finally:
        lib.emg3d_set_option(b'line_lpw', old)
    a = e0.copy()
    ocore.gauss_seidel_y(a.fx, a.fy, a.fz, *args, order=1)
    assert relerr(out[lpw], a.field) < 2e-12
    assert np.array_equal(out[lpw], out[0])


RAGGED_SOLVES = [
    ((48, 32, 24), dict(cycle='W', semicoarsening=True, linerelaxation=True)),
    ((24, 40, 16), dict(cycle='V', semicoarsening=2, linerelaxation=2)),
    ((20, 12, 36), dict(cycle='F', semicoarsening=False, linerelaxation=7, clevel=1)),
]


def _ragged_problem(shape, freq=0.8, sources=((3., -2., 1., 20., 30.),)):
    """Stretched non-cubic grid with a random tri-axial model: (grid, model, source fields, oracle volume model)."""
    rng = np.random.default_rng(sum(shape))
    h = [widths(n // 2, n // 4, 20., 1.15) for n in shape]
    grid = emg3d.TensorMesh(h, [-w.sum() / 2 for w in h])
    assert grid.shape_cells == shape
    rho = 10 ** rng.uniform(-0.5, 1.0, shape)
    model = emg3d.Model(grid, rho, 1.5 * rho, 2.5 * rho)
    sfields = [emg3d.get_source_field(grid, src, freq) for src in sources]
    ogrid = mg_ref.Grid(grid.h, grid.origin)
    vm = mg_ref.volume_model(ogrid, freq, 1 / rho, 1 / (1.5 * rho), 1 / (2.5 * rho))
    return grid, model, sfields, vm


@pytest.mark.parametrize('shape,kw', RAGGED_SOLVES)
def test_solve_ragged_grids_vs_oracle(shape, kw):
    """Non-cubic grids whose coarsest levels are odd (3, 5, 9 cells) or stop early: GPU
    vs oracle (lexicographic) converged fields, tri-axial random model; and the cycle count of the oracle's
    driver in the GPU's own smoother ordering."""
    grid, model, (sfield,), vm = _ragged_problem(shape)
    e, info = emg3d.solve(model, sfield, sslsolver=False, tol=1e-10, return_info=True, **kw)
    assert info['exit'] == 0, info['exit_message']
    ogrid = vm.grid
    eo, io = mg_ref.solve(vm, mg_ref.Field(ogrid, sfield.field.copy()), tol=1e-10, **kw)
    assert io['exit'] == 0
    assert relerr(e.field, eo.field) < 1e-8
    _, io1 = mg_ref.solve(vm, mg_ref.Field(ogrid, sfield.field.copy()), tol=1e-10, order=1, **kw)
    assert io1['exit'] == 0
    assert info['it_mg'] == io1['it_mg']


def _one_cycle_on(model, sfields, vm, **kw):
    """ONE multigrid cycle (fp64 line records) of `model` for the source field(s) -- a list goes through
    solve_batch -- on the GPU and with the oracle's driver on its volume model `vm` in the same smoother ordering,
    with the assertions of the fp64 branch of _one_cycle_vs_oracle: fields after the cycle to 1e-10, residual norms
    to 1e-9, the same smoother work. A transfer, a coarse model or a residual that is slightly wrong shows here
    (it does not in a converged field: the fixed point is the same)."""
    if isinstance(sfields, (list, tuple)):
        got = emg3d.solve_batch(model, list(sfields), tol=1e-30, maxit=1, line_compact=False, **kw)
    else:
        sfields = [sfields]
        got = [emg3d.solve(model, sfields[0], sslsolver=False, tol=1e-30, maxit=1, return_info=True,
                           line_compact=False, **kw)]
    assert len(got) == len(sfields)
    for b, ((e, info), sf) in enumerate(zip(got, sfields)):
        eo, io = mg_ref.solve(vm, mg_ref.Field(vm.grid, sf.field.copy()), tol=1e-30, maxit=1, order=1, **kw)
        assert info['it_mg'] == io['it_mg'] == 1
        d = relerr(e.field, eo.field)
        print(f"one cycle {vm.grid.shape_cells} {kw} source {b}: field {d:.2e}, abs_error {info['abs_error']:.6e} "
              f"(oracle {io['abs_error']:.6e}, rel {abs(info['abs_error'] / io['abs_error'] - 1):.2e})")
        assert np.linalg.norm(eo.field) > 0 and e.field.dtype == eo.field.dtype
        assert d < 1e-10, (b, d)
        assert info['abs_error'] == pytest.approx(io['abs_error'], rel=1e-9), b
        assert info['smoother_cell_sweeps'] == io['smooth_work'], b


@pytest.mark.parametrize('shape,kw', RAGGED_SOLVES)
def test_ragged_grids_one_cycle_vs_oracle_same_order(shape, kw):
    """The grids and options of test_solve_ragged_grids_vs_oracle (W-cycle with rotating semicoarsening and line
    relaxation; V-cycle, y never coarsened, y-lines; F-cycle, three line directions, one coarse level): ONE cycle
    against the oracle in the same ordering -- coarse levels of odd and 2-cell directions, every transfer of the
    cycle compared before convergence hides it."""
    grid, model, (sfield,), vm = _ragged_problem(shape)
    _one_cycle_on(model, sfield, vm, **kw)


def test_ragged_grid_one_cycle_laplace_domain_vs_oracle_same_order():
    """One F-cycle with semicoarsening and line relaxation in the Laplace domain (real arithmetic: the <double>
    instantiations of every kernel of the cycle) on the 48 x 32 x 24 grid."""
    grid, model, (sfield,), vm = _ragged_problem((48, 32, 24), freq=-0.8)
    assert sfield.field.dtype == np.float64 and vm.eta_x.dtype == np.float64
    _one_cycle_on(model, sfield, vm, cycle='F', semicoarsening=True, linerelaxation=True)


def test_ragged_grid_one_cycle_batch_of_three_vs_oracle_same_order():
    """solve_batch of three sources on 48 x 32 x 24, one W-cycle: every source against the oracle's cycle for that
    source alone (the batch strides of the residual, restriction and prolongation launches on every level)."""
    sources = ((3., -2., 1., 20., 30.), (-40., 25., -10., 70., -15.), (10., 10., 5., 0., 90.))
    grid, model, sfields, vm = _ragged_problem((48, 32, 24), sources=sources)
    _one_cycle_on(model, sfields, vm, cycle='W', semicoarsening=True, linerelaxation=True)


@pytest.mark.parametrize('shape', [(36, 20, 18), (40, 24, 33)])
@pytest.mark.parametrize('dtype,extras', [(complex, False), (float, False), (complex, True)])
def test_point_tiled_compact_eta_sums_vs_cpu_walk(shape, dtype, extras):
    """The tiled point smoother with its eta edge sums stored in SINGLE precision (emg3d_level flag POINT_COMPACT:
    levels that solve a correction equation; 4-byte halves where eta is purely imaginary or the field real, 8-byte
    pairs with epsilon_r): per sweep against the CPU walk of the same kernel bodies with the same storage (tests/emu,
    launch.h tile_pst_setup / tile_pst_load: the sums are plain additions, both sides round the same doubles) at the
    per-sweep tolerance, and against the fp64 sums: different (the storage is narrower), close (6e-8 of the diagonals'
    conduction parts)."""
    from emu import emu
    lib = _lib.lib()
    grid, vm, s, e0 = _random_level_fields(shape, dtype, sum(shape) + 3, freq=3e6 if extras else 1.3, extras=extras)
    dev = torch.device('cuda')
    nu = 3 if (extras and dtype is complex) else 1      # (the CPU walk's rule: full values for nu = 3, 7, ..., halves for 1, 5, ...)
    out = {}
    with _option('point_tile_min', 1):
        for compact in (False, True):
            lv = DeviceLevel.from_host(vm, dev)
            if compact:
                lv.set_line_compact(True)
            assert bool(lib.emg3d_point_compact_used(lv._cref)) == compact
            lv.s.copy_(torch.from_numpy(s.field))
            lv.e.copy_(torch.from_numpy(e0.field))
            lv.smooth(0, nu)
            out[compact] = lv.e.cpu().numpy()
            nbytes = lv.point_factors().numel()
        assert nbytes * 2 == lib.emg3d_point_fac_bytes(*shape, int(dtype is complex)) // (1 if extras or dtype is float else 2)
    ref = e0.copy()
    emu.lib().emu_set_point_tile_min(1)
    emu.lib().emu_set_point_compact(1)
    try:
        emu.gauss_seidel(ref, s, vm, 0, nu)
    finally:
        emu.lib().emu_set_point_compact(0)
        emu.lib().emu_set_point_tile_min(1 << 20)
    d = relerr(out[True], out[False])
    assert relerr(out[True], ref.field) < 5e-10, relerr(out[True], ref.field)      # (tolerance of the fp64 test below)
    assert 1e-12 < d < 1e-5, d


@pytest.mark.parametrize('shape', [(36, 20, 18), (16, 8, 8), (18, 34, 10), (40, 24, 33)])
@pytest.mark.parametrize('dtype,extras', [(complex, False), (float, False), (complex, True), (float, True)])
def test_point_tiled_schedule_vs_oracle_tile_order(shape, dtype, extras):
    """Tiled point smoother (k_gs_point_tile: LDS tile, eight tile colours) forced on small
    grids with several / partial tiles, against the oracle's order 2; with the precomputed
    eta edge sums (host flavour) and with sums formed on the fly (device flavour, fac = NULL)."""
    lib = _lib.lib()
    rng = np.random.default_rng(sum(shape))
    h = [rng.uniform(0.5, 2.0, n) for n in shape]
    grid = mg_ref.Grid(h, (0., 0., 0.))
    sig = [10 ** rng.uniform(-1, 1, shape) for _ in range(3)]
    # extras: epsilon_r / mu_r at 3 MHz -- eta with a real part (the tiled kernel's full-width eta-sum
    # layout, emg3d_level::flags without ETA_IMAG), zeta = V / mu_r
    kwx = dict(mu_r=rng.uniform(0.7, 3.0, shape), epsilon_r=rng.uniform(1., 80., shape)) if extras else {}
    fq = 3e6 if extras else 1.3
    vm = mg_ref.volume_model(grid, fq if dtype is complex else -fq, *sig, **kwx)
    if extras and dtype is complex:
        assert np.abs(vm.eta_x.real).max() > 1e-3 * np.abs(vm.eta_x.imag).max()
    s = mg_ref.Field(grid, dtype=dtype)
    e0 = mg_ref.Field(grid, dtype=dtype)
    for f in (s, e0):
        f.field[:] = rng.standard_normal(f.field.size)
        if dtype is complex:
            f.field[:] += 1j * rng.standard_normal(f.field.size)
    for f in (e0.fx[:, 0, :], e0.fx[:, -1, :], e0.fx[:, :, 0], e0.fx[:, :, -1], e0.fy[0], e0.fy[-1],
              e0.fy[:, :, 0], e0.fy[:, :, -1], e0.fz[0], e0.fz[-1], e0.fz[:, 0], e0.fz[:, -1]):
        f[...] = 0
    lib.emg3d_set_option(b'point_tile_min', 1)
    try:
        for nu in (1, 2):
            a, b = e0.copy(), e0.copy()
            ocore.gauss_seidel(a.fx, a.fy, a.fz, s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z,
                               vm.zeta, *grid.h, nu, order=2)
            core.gauss_seidel(b.fx, b.fy, b.fz, s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z,
                              vm.zeta, *grid.h, nu)
            assert relerr(b.field, a.field) < 5e-10, (shape, nu)
            # device flavour without the eta-sum buffer
            lv = DeviceLevel.from_host(vm, torch.device('cuda'))
            assert bool(lv.flags & _lib.LEVEL_ETA_IMAG) == (dtype is complex and not extras)
            lv.s.copy_(torch.from_numpy(s.field))
            lv.e.copy_(torch.from_numpy(e0.field))
            _lib.check(lib.emg3d_dev_gauss_seidel(lv._cref, 0, nu, None, None, None, 0, None), 'gs')
            torch.cuda.synchronize()
            assert np.array_equal(lv.e.cpu().numpy(), b.field), (shape, nu)
    finally:
        lib.emg3d_set_option(b'point_tile_min', 1 << 20)


def test_solve_with_tiled_point_smoother_vs_oracle():
    """Whole solves with the tiled order forced on every level (point_tile_min = 1): same
    cycle count and converged field as the oracle run with the same rule."""
    lib = _lib.lib()
    shape = (40, 24, 32)
    rng = np.random.default_rng(11)
    h = [widths(n // 2, n // 4, 20., 1.1) for n in shape]
    grid = emg3d.TensorMesh(h, [-w.sum() / 2 for w in h])
    rho = 10 ** rng.uniform(-0.5, 1.0, shape)
    model = emg3d.Model(grid, rho, 1.5 * rho, 2.5 * rho)
    sfield = emg3d.get_source_field(grid, (3., -2., 1., 20., 30.), 0.8)
    ogrid = mg_ref.Grid(grid.h, grid.origin)
    vm = mg_ref.volume_model(ogrid, 0.8, 1 / rho, 1 / (1.5 * rho), 1 / (2.5 * rho))
    lib.emg3d_set_option(b'point_tile_min', 1)
    try:
        e, info = emg3d.solve(model, sfield, sslsolver=False, semicoarsening=False,
                              linerelaxation=False, cycle='F', tol=1e-10, return_info=True)
    finally:
        lib.emg3d_set_option(b'point_tile_min', 1 << 20)
    eo, io = mg_ref.solve(vm, mg_ref.Field(ogrid, sfield.field.copy()), tol=1e-10, cycle='F',
                          order=1, tile_min=1)
    assert info['exit'] == 0 and io['exit'] == 0
    assert info['it_mg'] == io['it_mg']
    assert relerr(e.field, eo.field) < 1e-8


def test_bench_workload_marine64_converged_vs_oracle():
    """BASELINE.json config 2 at half size (bench.py workload 'marine64': stretched marine
    halfspace, VTI, F-cycle + semicoarsening + line relaxation): converged field of the GPU
    path vs the oracle in the reference's lexicographic order, both at tol 1e-10 -> 1e-8."""
    from bench import workload
    wl = workload('marine64')
    grid = emg3d.TensorMesh(wl['h'], wl['origin'])
    model = emg3d.Model(grid, **wl['res'])
    sfield = emg3d.get_source_field(grid, wl['source'], wl['frequency'])
    e, info = emg3d.solve(model, sfield, sslsolver=False, tol=1e-10, return_info=True, **wl['opts'])
    assert info['exit'] == 0, info['exit_message']
    ogrid = mg_ref.Grid(grid.h, grid.origin)
    cond = {k: 1.0 / np.asarray(v, dtype=float) for k, v in wl['res'].items()}
    vm = mg_ref.volume_model(ogrid, wl['frequency'], cond['property_x'], None, cond['property_z'])
    eo, io = mg_ref.solve(vm, mg_ref.Field(ogrid, sfield.field.copy()), tol=1e-10, **wl['opts'])
    assert io['exit'] == 0
    assert relerr(e.field, eo.field) < 1e-8
    assert abs(info['it_mg'] - io['it_mg']) <= 3


@pytest.mark.parametrize('freq', [1.0, 0.01, -3.0])
def test_line_smoothers_low_frequency_accuracy(freq):
    """The two-sided line factorisation must keep the accuracy of the reference's one-sided
    LDL^T when the blocks are nearly singular (low frequency: the gradient null space of the
    curl-curl operator is only weakly regularised). Eliminating the far half in the
    reference's block grouping loses accuracy like cond^2 (2e-8 at 0.01 Hz); the mirrored
    grouping of stencil.h keeps cond * eps."""
    shape = (64, 6, 10)
    rng = np.random.default_rng(1)
    h = [np.ones(n) * 20. for n in shape]
    grid = mg_ref.Grid(h, (0., 0., 0.))
    sig = [10 ** rng.uniform(-1, 1, shape) for _ in range(3)]
    vm = mg_ref.volume_model(grid, freq, *sig)
    dtype = complex if freq > 0 else float
    s = mg_ref.Field(grid, dtype=dtype)
    e0 = mg_ref.Field(grid, dtype=dtype)
    for f in (s, e0):
        f.field[:] = rng.standard_normal(f.field.size)
        if dtype is complex:
            f.field[:] += 1j * rng.standard_normal(f.field.size)
    for f in (e0.fx[:, 0, :], e0.fx[:, -1, :], e0.fx[:, :, 0], e0.fx[:, :, -1], e0.fy[0], e0.fy[-1],
              e0.fy[:, :, 0], e0.fy[:, :, -1], e0.fz[0], e0.fz[-1], e0.fz[:, 0], e0.fz[:, -1]):
        f[...] = 0
    tol = {1.0: 2e-12, 0.01: 2e-10, -3.0: 2e-11}[freq]
    for fn in ('gauss_seidel_x', 'gauss_seidel_y', 'gauss_seidel_z'):
        a, b = e0.copy(), e0.copy()
        getattr(ocore, fn)(a.fx, a.fy, a.fz, s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z,
                           vm.zeta, *grid.h, 1, order=1)
        getattr(core, fn)(b.fx, b.fy, b.fz, s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z,
                          vm.zeta, *grid.h, 1)
        assert relerr(b.field, a.field) < tol, (fn, freq)


@pytest.mark.parametrize('freq', [1.3, -2.5])
@pytest.mark.parametrize('case', ['isotropic', 'VTI', 'HTI', 'triaxial'])
def test_volume_model_device_arrays_match_host(case, freq):
    """solve() forms eta / zeta directly in HBM (VolumeModel.device_arrays); they must equal
    the host formulas of the reference (emg3d/models.py:654-691), including epsilon_r, mu_r,
    the Laplace domain and the aliasing of eta_y / eta_z."""
    rng = np.random.default_rng(3)
    shape = (6, 5, 7)
    grid = emg3d.TensorMesh([rng.uniform(1, 3, n) for n in shape], (0., 0., 0.))
    kw = dict(property_x=10 ** rng.uniform(-1, 1, shape), mu_r=rng.uniform(1, 2, shape),
              epsilon_r=rng.uniform(1, 80, shape))
    if case in ('HTI', 'triaxial'):
        kw['property_y'] = 10 ** rng.uniform(-1, 1, shape)
    if case in ('VTI', 'triaxial'):
        kw['property_z'] = 10 ** rng.uniform(-1, 1, shape)
    for drop in ((), ('mu_r',), ('epsilon_r',), ('mu_r', 'epsilon_r')):
        model = emg3d.Model(grid, **{k: v for k, v in kw.items() if k not in drop})
        sfield = emg3d.Field(grid, frequency=freq)
        vm = emg3d.models.VolumeModel(model, sfield)
        ex, ey, ez, zeta = vm.device_arrays(torch.device('cuda'))
        assert (ey is ex) == (vm.eta_y is vm.eta_x) and (ez is ex) == (vm.eta_z is vm.eta_x)
        for dev, host in ((ex, vm.eta_x), (ey, vm.eta_y), (ez, vm.eta_z), (zeta, vm.zeta)):
            got = dev.cpu().numpy()
            assert got.dtype == host.dtype
            assert relerr(got, host.ravel('F')) < 1e-15, (case, freq, drop)


def test_parallel_compute_concurrent_solves_per_gpu():
    """parallel.compute(per_gpu=2): two solves at a time on one GPU (own host threads and HIP
    streams) give the fields of the one-after-the-other run."""
    from emg3d_amd import parallel
    hx = widths(8, 4, 50., 1.2)
    grid = emg3d.TensorMesh([hx, hx, hx], (-hx.sum() / 2,) * 3)
    rng = np.random.default_rng(5)
    model = emg3d.Model(grid, 10 ** rng.uniform(-0.5, 0.5, grid.shape_cells))
    sources = {f'S{i}': (-40. + 30. * i, 0., 10., 0., 0.) for i in range(4)}
    freqs = {'f1': 1.0, 'f2': 3.0}
    opts = {'sslsolver': False, 'tol': 1e-8, 'verb': 0}
    seq = parallel.compute(model, grid, sources, freqs, opts, reuse=False)
    con = parallel.compute(model, grid, sources, freqs, opts, per_gpu=3)
    reu = parallel.compute(model, grid, sources, freqs, opts)      # shared hierarchies per frequency
    keys = sorted(k for k in seq if k != '_all_info')
    assert sorted(k for k in con if k != '_all_info') == keys and len(keys) == 8
    for k in keys:
        assert seq[k][1]['exit'] == 0 and con[k][1]['exit'] == 0
        assert con[k][1]['it_mg'] == seq[k][1]['it_mg'] == reu[k][1]['it_mg']
        assert np.array_equal(con[k][0].field, seq[k][0].field), k
        assert np.array_equal(reu[k][0].field, seq[k][0].field), k


def test_solve_with_reused_hierarchy():
    """solve(hierarchy=...): several sources at one frequency on one set of device-resident
    levels / line factors / graphs -- same fields as separate solves, default BiCGSTAB and plain
    multigrid; a hierarchy of another frequency is refused."""
    hx = widths(8, 4, 50., 1.2)
    grid = emg3d.TensorMesh([hx, hx, hx[:12]], (-hx.sum() / 2, -hx.sum() / 2, -300.))
    rng = np.random.default_rng(11)
    model = emg3d.Model(grid, 10 ** rng.uniform(-0.5, 0.5, grid.shape_cells),
                        property_z=10 ** rng.uniform(0, 0.5, grid.shape_cells))
    sfields = [emg3d.get_source_field(grid, (x, 5., -100., 10., 5.), 0.7) for x in (-60., 0., 45.)]
    hier = solver.Hierarchy(emg3d.models.VolumeModel(model, sfields[0]))
    for kw in (dict(sslsolver=False), dict()):
        for sf in sfields:
            e1, i1 = emg3d.solve(model, sf, return_info=True, tol=1e-9, **kw)
            e2, i2 = emg3d.solve(model, sf, return_info=True, tol=1e-9, hierarchy=hier, **kw)
            assert i1['exit'] == 0 and i1['it_mg'] == i2['it_mg'] and i1['it_ssl'] == i2['it_ssl']
            assert np.array_equal(e1.field, e2.field)
    other = emg3d.get_source_field(grid, (0., 0., -100., 0., 0.), 2.0)
    with pytest.raises(ValueError, match='hierarchy'):
        emg3d.solve(model, other, hierarchy=hier)


def test_rccl_single_rank_model_broadcast():
    """The collectives of the multi-GPU job (RCCL through torch.distributed 'nccl') on the
    one GPU of this box: a world of one rank runs init, the model broadcast of
    parallel.broadcast_model's tensor path, all-reduce and barrier. The sharding logic itself
    is covered with two gloo processes in tests/test_parallel_gloo.py."""
    import subprocess
    import sys
    code = (
        "import os, sys, torch, numpy as np\n"
        "import torch.distributed as dist\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from emg3d_amd import parallel\n"
        "os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT='29533')\n"
        "dev = torch.device('cuda', 0); torch.cuda.set_device(dev)\n"
        "dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)\n"
        "t = torch.arange(1000, dtype=torch.float64)\n"
        "t = parallel._bcast_tensor(t, 0, dev)\n"
        "assert t.is_cuda and float(t.sum()) == 499500.0\n"
        "m = torch.tensor([3.0, 4.0], dtype=torch.float64, device=dev)\n"
        "dist.all_reduce(m, op=dist.ReduceOp.MAX); dist.barrier(); torch.cuda.synchronize()\n"
        "assert m.tolist() == [3.0, 4.0]\n"
        "assert parallel.gather_objects({'a': 1}) == [{'a': 1}]\n"
        "parallel.finalize(); print('rccl ok')\n")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and 'rccl ok' in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize('seed', range(18))
def test_randomised_smoother_parity(seed):
    """Randomised sweep over grid shapes (even, odd, 2-cell, long and short lines: every
    middle-block position and padding of the two-sided line solve, every lines-per-workgroup /
    LDS-record mode of the fused kernel), anisotropy cases, dtypes and sweep counts: each
    smoother on the GPU against the oracle in the same ordering, per call."""
    rng = np.random.default_rng(1000 + seed)
    shape = tuple(int(rng.choice([2, 3, 4, 5, 6, 8, 9, 12, 16, 17, 24, 33, 40, 70])) for _ in range(3))
    if np.prod(shape) > 60000:
        shape = (shape[0], min(shape[1], 12), min(shape[2], 16))
    case = str(rng.choice(['isotropic', 'VTI', 'HTI', 'triaxial']))
    freq = float(rng.choice([1.0, 0.1, -1.0]))
    h = [rng.uniform(5., 15., n) * 1.1 ** np.abs(np.arange(n) - n // 2) for n in shape]
    grid = mg_ref.Grid(h, (0., 0., 0.))
    sx = 10 ** rng.uniform(-1, 1, shape)
    sy = 10 ** rng.uniform(-1, 1, shape) if case in ('HTI', 'triaxial') else None
    sz = 10 ** rng.uniform(-1, 1, shape) if case in ('VTI', 'triaxial') else None
    # every third case with epsilon_r and mu_r at a frequency where the displacement term matters: eta gets a
    # real part of the size of its imaginary one (emg3d/models.py:677-691), zeta = V / mu_r
    extras = {}
    if seed % 3 == 2:
        freq = 2e6 if freq > 0 else -2e6
        extras = dict(mu_r=rng.uniform(0.7, 3.0, shape), epsilon_r=rng.uniform(1., 80., shape))
    vm = mg_ref.volume_model(grid, freq, sx, sy, sz, **extras)
    if extras and freq > 0:
        assert np.abs(vm.eta_x.real).max() > 1e-3 * np.abs(vm.eta_x.imag).max()
    dtype = complex if freq > 0 else float
    s = mg_ref.Field(grid, dtype=dtype)
    e0 = mg_ref.Field(grid, dtype=dtype)
    for f in (s, e0):
        f.field[:] = rng.standard_normal(f.field.size)
        if dtype is complex:
            f.field[:] += 1j * rng.standard_normal(f.field.size)
    for f in (e0.fx[:, 0, :], e0.fx[:, -1, :], e0.fx[:, :, 0], e0.fx[:, :, -1], e0.fy[0], e0.fy[-1],
              e0.fy[:, :, 0], e0.fy[:, :, -1], e0.fz[0], e0.fz[-1], e0.fz[:, 0], e0.fz[:, -1]):
        f[...] = 0
    nu = int(rng.integers(1, 4))
    for fn in SMOOTHERS:
        a, b = e0.copy(), e0.copy()
        getattr(ocore, fn)(a.fx, a.fy, a.fz, s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z,
                           vm.zeta, *grid.h, nu, order=1)
        getattr(core, fn)(b.fx, b.fy, b.fz, s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z,
                          vm.zeta, *grid.h, nu)
        assert relerr(b.field, a.field) < 1e-10, (shape, case, freq, nu, fn)


def test_magnetic_field_and_receivers_vs_reference_vectors(golden_receivers):
    """SURVEY.md 8f rank 2 on the device: get_magnetic_field (emg3d/fields.py:617-659) and
    get_receiver (emg3d/fields.py:522-614; cubic and linear) against the reference's outputs
    for random fields: electric and magnetic, frequency and Laplace domain; receivers on
    nodes, inside, in the outermost cells (NaN) and outside (NaN)."""
    g = golden_receivers
    grid = emg3d.TensorMesh([g['hx'], g['hy'], g['hz']], g['origin'])
    model = emg3d.Model(grid, property_x=g['property_x'], mu_r=g['mu_r'])
    rec = (g['rec_x'], g['rec_y'], g['rec_z'], g['rec_azimuth'], g['rec_elevation'])
    for tag in ('f', 's'):
        efield = emg3d.Field(grid, data=g[tag + '_efield'], frequency=float(g[tag + '_frequency']))
        hfield = emg3d.get_magnetic_field(model, efield)
        assert not hfield.electric and hfield.fx.shape == grid.shape_faces_x
        assert hfield.field.dtype == g[tag + '_hfield'].dtype
        assert relerr(hfield.field, g[tag + '_hfield']) < 1e-13
        assert np.all(hfield.fx[0] == 0) and np.all(hfield.fz[:, :, -1] == 0)      # boundary faces
        for kind, fld in (('e', efield), ('h', hfield)):
            for method in ('cubic', 'linear'):
                got = fld.get_receiver(rec, method=method)
                want = g[f'{tag}_{kind}_{method}']
                m = np.isnan(want)
                assert got.shape == want.shape and got.dtype == want.dtype
                assert np.array_equal(m, np.isnan(got)), (tag, kind, method)
                assert np.abs(got[~m] - want[~m]).max() <= 1e-11 * np.abs(want[~m]).max(), (tag, kind, method)
    # scalar coordinates -> 0-d result; bad input
    one = efield.get_receiver((float(rec[0][8]), float(rec[1][8]), float(rec[2][8]), 0., 0.))
    assert one.shape == () and np.isfinite(one)
    with pytest.raises(ValueError, match='receiver'):
        emg3d.get_receiver(efield, (1., 2., 3.))


def test_spline_and_linear_device_kernels_vs_scipy():
    """The device spline prefilter and the spline evaluation against SciPy itself on a 96 x 70 x 50
    array (complex and real), coordinates up to and beyond the edges. The trilinear kernel is not
    called here: test_pre_post_kernels.py::test_linear_eval_kernel_vs_scipy calls it directly."""
    import scipy.ndimage as ndi
    from emg3d_amd._device import _ptr, _stream
    rng = np.random.default_rng(3)
    shape = (96, 70, 50)
    n = 500
    coords = np.array([rng.uniform(-2, s + 1, n) for s in shape])
    coords[:, :4] = np.array([[0, 0, 0], [95, 69, 49], [0.01, 68.99, 25], [94.5, 0.5, 48.7]]).T
    dev = torch.device('cuda')
    lib = _lib.lib()
    for dtype in (complex, float):
        v = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if dtype is complex else 0)
        v = np.asfortranarray(v.astype(dtype))
        ref = ndi.map_coordinates(v, coords, order=3, mode='constant', cval=np.nan)
        d = torch.from_numpy(v.ravel('F').copy()).to(dev)
        dc = torch.from_numpy(coords.copy()).to(dev)
        out = torch.empty(n, dtype=d.dtype, device=dev)
        _lib.check(lib.emg3d_dev_spline_filter(_ptr(d), *shape, int(dtype is complex), _stream()))
        coef = ndi.spline_filter(v.real, order=3, mode='constant')
        got_coef = d.cpu().numpy().reshape(shape, order='F')
        assert np.abs(got_coef.real - coef).max() < 1e-12
        _lib.check(lib.emg3d_dev_spline_eval(_ptr(d), *shape, int(dtype is complex), _ptr(dc), n, _ptr(out), _stream()))
        got = out.cpu().numpy()
        m = np.isnan(ref)
        assert np.array_equal(m, np.isnan(got)) and 0 < m.sum() < n
        assert np.abs(got[~m] - ref[~m]).max() < 1e-12


def test_parallel_compute_responses_from_device_field():
    """parallel.compute(receivers=...): responses interpolated from the solution while it is in
    HBM equal get_receiver() on the downloaded fields; with keep_fields=False no field comes
    back; multigrid and the default BiCGSTAB."""
    from emg3d_amd import parallel
    hx = widths(8, 4, 50., 1.2)
    grid = emg3d.TensorMesh([hx, hx, hx], (-hx.sum() / 2,) * 3)
    rng = np.random.default_rng(8)
    model = emg3d.Model(grid, 10 ** rng.uniform(-0.5, 0.5, grid.shape_cells))
    sources = {f'S{i}': (-40. + 30. * i, 0., 10., 0., 0.) for i in range(3)}
    freqs = {'f1': 1.0}
    rec = (rng.uniform(-150, 150, 9), rng.uniform(-150, 150, 9), rng.uniform(-100, 100, 9),
           rng.uniform(-180, 180, 9), rng.uniform(-30, 30, 9))
    for ssl in (False, True):
        opts = {'sslsolver': ssl, 'tol': 1e-8, 'verb': 0}
        full = parallel.compute(model, grid, sources, freqs, opts, receivers=rec)
        lean = parallel.compute(model, grid, sources, freqs, opts, receivers=rec, keep_fields=False,
                                receiver_method='linear')
        for k in [k for k in full if k != '_all_info']:
            want = full[k][0].get_receiver(rec)
            assert np.all(np.isfinite(want))
            assert np.array_equal(full[k][1]['responses'], want)
            assert lean[k][0] is None
            assert np.array_equal(lean[k][1]['responses'], full[k][0].get_receiver(rec, method='linear'))
        assert set(full['_all_info'][('S0', 'f1')]) >= {'responses', 'it_mg'}


def test_parallel_compute_magnetic_receivers_from_device_field():
    """`parallel.compute(receivers=..., magnetic=...)`: electric and magnetic point receivers; the
    magnetic responses are formed on the device (H from the solution in HBM, then the interpolation)
    and equal `get_receiver(get_magnetic_field(model, efield), ...)` of the downloaded field."""
    from emg3d_amd import parallel
    hx = widths(8, 3, 50., 1.3)
    grid = emg3d.TensorMesh([hx, hx, hx], (-hx.sum() / 2,) * 3)
    model = emg3d.Model(grid, property_x=np.full(grid.shape_cells, 1.5))
    rec = (np.array([120., -80., 40.]), np.array([30., 60., -90.]), np.array([-20., 10., 55.]),
           np.array([0., 90., 30.]), np.array([0., 0., 45.]))
    mag = np.array([False, True, True])
    srcs, freqs = {'s': (0., 0., 0., 0., 0.)}, {'f': 1.0}
    opts = dict(sslsolver=False, cycle='F', semicoarsening=True, linerelaxation=True, tol=1e-8)
    for keep in (True, False):
        out = parallel.compute(model, grid, srcs, freqs, solver_opts=opts, receivers=rec, magnetic=mag,
                               keep_fields=keep, receiver_method='cubic')
        ef, info = out[('s', 'f')]
        resp = info['responses']
        assert (ef is None) == (not keep)
        if keep:
            want = np.array(emg3d.fields.get_receiver(ef, rec, 'cubic'))
            want[mag] = emg3d.fields.get_receiver(emg3d.get_magnetic_field(model, ef), tuple(c[mag] for c in rec), 'cubic')
            first = resp
            assert np.allclose(resp, want, rtol=1e-12, atol=0)
        else:
            assert np.allclose(resp, first, rtol=1e-12, atol=0)


def test_model_regridding_vs_reference_vectors(golden_gridding):
    """Model.interpolate_to_grid (volume averaging on the device) against
    models re-gridded by the reference; the same grid returns the model itself; a solve on the
    re-gridded model runs."""
    g = golden_gridding
    mesh = lambda t: emg3d.TensorMesh([g[f'{t}_hx'], g[f'{t}_hy'], g[f'{t}_hz']], g[f'{t}_origin'])   # noqa: E731
    grid = mesh('in')
    for mapping in ('Resistivity', 'Conductivity', 'LgConductivity'):
        props = {p: g[f'{mapping}_in_{p}'] for p in ('property_x', 'property_z', 'mu_r', 'epsilon_r')}
        model = emg3d.Model(grid, mapping=mapping, **props)
        assert model.interpolate_to_grid(mesh('in')) is model
        for t in ('fine', 'coarse', 'same_nodes'):
            new = model.interpolate_to_grid(mesh(t))
            assert new.mapping == mapping and new.case == 'VTI' and new.property_y is None
            for p in props:
                want = g[f'{mapping}_{t}_{p}']
                got = getattr(new, p)
                assert got.shape == want.shape
                assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), (mapping, t, p)
    with pytest.raises(NotImplementedError):
        model.interpolate_to_grid(mesh('fine'), method='cubic')
    # the worker path: model on one grid, computation on another
    from emg3d_amd import parallel
    model = emg3d.Model(grid, property_x=g['Resistivity_in_property_x'])
    comp = emg3d.TensorMesh([np.full(16, 80.), np.full(16, 90.), np.full(8, 100.)], (-640., -720., -700.))
    e, info = parallel.solve({'model': model, 'grid': comp, 'source': (0., 0., -300., 0., 0.), 'frequency': 1.0,
                              'efield': None, 'solver_opts': {'tol': 1e-6}})
    assert info['exit'] == 0 and e.grid == comp


@pytest.mark.parametrize('kw', [dict(), dict(cycle='W', linerelaxation=False), dict(plain=True, cycle='V'),
                                dict(semicoarsening=False, linerelaxation=2), dict(residual_form=True)])
def test_solve_batch_equals_separate_solves(kw):
    """solve_batch: several sources of one frequency through the same launches (emg3d_level::batch)
    give, source by source, the field, cycle count and error history of separate solves -- also
    when the sources need different numbers of cycles."""
    hx = widths(8, 4, 50., 1.2)
    grid = emg3d.TensorMesh([hx, hx[:12], hx], (-hx.sum() / 2, -330., -hx.sum() / 2))
    rng = np.random.default_rng(21)
    model = emg3d.Model(grid, 10 ** rng.uniform(-0.5, 0.5, grid.shape_cells),
                        property_z=10 ** rng.uniform(0, 0.7, grid.shape_cells))
    srcs = [(-120., 20., -40., 0., 0.), (30., -60., 10., 45., 10.), (0., 0., 0., 90., 0.),
            ([-200., 150.], [-100., 90.], [-30., 60.])]
    sfields = [emg3d.get_source_field(grid, s if len(s) == 5 else np.array(s).T, 0.9) for s in srcs]
    sfields[2].field *= 1e-3           # a weaker source: same relative tolerance, other history
    sfields[2]._sparse = None
    sep = [emg3d.solve(model, sf, sslsolver=False, tol=1e-7, return_info=True, **kw) for sf in sfields]
    bat = emg3d.solve_batch(model, sfields, tol=1e-7, **kw)
    assert len(bat) == len(sep)
    for (e1, i1), (e2, i2) in zip(sep, bat):
        assert i1['exit'] == i2['exit'] == 0 and i1['it_mg'] == i2['it_mg']
        assert np.array_equal(i1['error_at_cycle'], i2['error_at_cycle'])
        assert i1['smoother_cell_sweeps'] == i2['smoother_cell_sweeps']
        assert np.array_equal(e1.field, e2.field)
    with pytest.raises(ValueError, match='share grid and frequency'):
        emg3d.solve_batch(model, [sfields[0], emg3d.get_source_field(grid, srcs[0], 2.0)])


def test_parallel_compute_batched_pairs():
    """parallel.compute(batch=4): the pairs of one frequency go through solve_batch; fields,
    cycle counts and device-side responses equal the pair-by-pair run; two frequencies and a
    ragged last batch."""
    from emg3d_amd import parallel
    hx = widths(8, 4, 50., 1.2)
    grid = emg3d.TensorMesh([hx, hx, hx], (-hx.sum() / 2,) * 3)
    rng = np.random.default_rng(5)
    model = emg3d.Model(grid, 10 ** rng.uniform(-0.5, 0.5, grid.shape_cells))
    sources = {f'S{i}': (-160. + 70. * i, 20. * i, 10., 15. * i, 0.) for i in range(5)}
    freqs = {'f1': 1.0, 'f2': 3.0}
    rec = (rng.uniform(-150, 150, 6), rng.uniform(-150, 150, 6), rng.uniform(-100, 100, 6), 0., 0.)
    opts = {'sslsolver': False, 'tol': 1e-8, 'verb': 0}
    seq = parallel.compute(model, grid, sources, freqs, opts, receivers=rec, reuse=False)
    bat = parallel.compute(model, grid, sources, freqs, opts, receivers=rec, batch=4)
    lean = parallel.compute(model, grid, sources, freqs, opts, receivers=rec, batch=3, keep_fields=False)
    keys = sorted(k for k in seq if k != '_all_info')
    assert sorted(k for k in bat if k != '_all_info') == keys and len(keys) == 10
    for k in keys:
        assert bat[k][1]['exit'] == 0 and bat[k][1]['it_mg'] == seq[k][1]['it_mg']
        assert np.array_equal(bat[k][0].field, seq[k][0].field), k
        assert np.array_equal(bat[k][1]['responses'], seq[k][1]['responses'])
        assert lean[k][0] is None and np.array_equal(lean[k][1]['responses'], seq[k][1]['responses'])
    # the default solver (BiCGSTAB + multigrid) in batches, and one that is not batched (gcrotmk)
    two = {k: sources[k] for k in ('S0', 'S1')}
    for o in ({'tol': 1e-7}, {'tol': 1e-7, 'sslsolver': 'cgs'}):
        a = parallel.compute(model, grid, two, {'f1': 1.0}, o, batch=2)
        b = parallel.compute(model, grid, two, {'f1': 1.0}, o)
        for k in (('S0', 'f1'), ('S1', 'f1')):
            assert a[k][1]['exit'] == b[k][1]['exit'] and a[k][1]['it_ssl'] == b[k][1]['it_ssl'] > 0
            assert 'sslsolver' in o or a[k][1]['exit'] == 0
            assert np.allclose(a[k][0].field, b[k][0].field, rtol=1e-6, atol=1e-6 * np.abs(b[k][0].field).max())


@pytest.mark.parametrize('kw', [dict(), dict(cycle='V', linerelaxation=False), dict(semicoarsening=False)])
def test_solve_batch_bicgstab(kw):
    """solve_batch(sslsolver=True): BiCGSTAB per source with shared multigrid preconditioner and
    operator applications -- same iteration counts as separate solves, and fields bit-identical (1e-12)
    while all sources run the same number of cycles per preconditioner call. When the sources of a batch
    need different numbers of Krylov iterations, the semicoarsening / line-relaxation cycling of the shared
    structure and of a separate solve drift apart (solver._bicgstab_batch): every source then still
    converges to the tolerance, and the fields agree to it."""
    hx = widths(8, 4, 50., 1.2)
    grid = emg3d.TensorMesh([hx, hx[:12], hx], (-hx.sum() / 2, -330., -hx.sum() / 2))
    rng = np.random.default_rng(31)
    model = emg3d.Model(grid, 10 ** rng.uniform(-0.5, 0.5, grid.shape_cells),
                        property_z=10 ** rng.uniform(0, 0.7, grid.shape_cells))
    sfields = [emg3d.get_source_field(grid, s, 0.9) for s in
               ((-120., 20., -40., 0., 0.), (30., -60., 10., 45., 10.), (0., 0., 0., 90., 0.))]
    sep = [emg3d.solve(model, sf, tol=1e-8, return_info=True, **kw) for sf in sfields]
    bat = emg3d.solve_batch(model, sfields, sslsolver=True, tol=1e-8, **kw)
    in_step = len({i['it_ssl'] for _, i in sep}) == 1          # all sources take the same number of iterations
    for (e1, i1), (e2, i2) in zip(sep, bat):
        assert i1['exit'] == i2['exit'] == 0
        if in_step:
            assert (i1['it_ssl'], i1['it_mg']) == (i2['it_ssl'], i2['it_mg'])
            assert np.allclose(i1['error_at_cycle'], i2['error_at_cycle'], rtol=1e-10)
            assert relerr(e2.field, e1.field) < 1e-12
        else:
            assert abs(i1['it_ssl'] - i2['it_ssl']) <= 1
            assert relerr(e2.field, e1.field) < 1e-7


@pytest.mark.parametrize('option,value', [('point_tile_min', 1), ('line_fuse', 0), ('line_lds', 0)])
def test_solve_batch_other_kernel_paths(option, value):
    """The batched instantiations that the default options do not reach on small grids: the
    tiled point smoother (forced by point_tile_min), the separate line launches (line_fuse = 0)
    and the fused line kernel with its records in the global scratch (line_lds = 0)."""
    lib = _lib.lib()
    old = lib.emg3d_get_option(option.encode())
    hx = widths(8, 4, 50., 1.2)
    grid = emg3d.TensorMesh([hx, hx[:12], hx], (-hx.sum() / 2, -330., -hx.sum() / 2))
    rng = np.random.default_rng(4)
    model = emg3d.Model(grid, 10 ** rng.uniform(-0.5, 0.5, grid.shape_cells))
    sfields = [emg3d.get_source_field(grid, (x, 10., -20., az, 0.), 1.1) for x, az in ((-90., 0.), (40., 60.), (0., 90.))]
    kw = dict(plain=True) if option == 'point_tile_min' else {}
    try:
        lib.emg3d_set_option(option.encode(), value)
        sep = [emg3d.solve(model, sf, sslsolver=False, tol=1e-7, return_info=True, **kw) for sf in sfields]
        bat = emg3d.solve_batch(model, sfields, tol=1e-7, **kw)
    finally:
        lib.emg3d_set_option(option.encode(), old)
    for (e1, i1), (e2, i2) in zip(sep, bat):
        assert i1['exit'] == i2['exit'] == 0 and i1['it_mg'] == i2['it_mg']
        assert np.array_equal(e1.field, e2.field)


@pytest.mark.parametrize('dtype', [complex, float])
def test_repeated_colour_pass_is_redundant(dtype):
    """Consecutive sweeps (backward, forward, ...) meet at one colour class; the second pass over
    it reproduces the values of the first bit by bit (its inputs, the edges off the lines / off
    the nodes, have not changed), so the library skips it (option skip_repeat = 1, default).
    All four smoothers, nu = 2, 3 and 4, with and without the pass: identical bits."""
    lib = _lib.lib()
    rng = np.random.default_rng(12)
    shape = (12, 10, 14)
    h = [widths(s - 4, 2, 30. + 7 * d, 1.3) for d, s in enumerate(shape)]
    grid = mg_ref.Grid(h, (0., 0., 0.))
    n = grid.n_cells
    sval = 2j * np.pi * 1.1 if dtype is complex else -1.7
    vol = (h[0][:, None, None] * h[1][None, :, None] * h[2][None, None, :])
    eta = [np.asfortranarray(-sval * 1.25663706127e-06 * vol * 10 ** rng.uniform(-1, 1, shape)).astype(dtype)
           for _ in range(3)]
    zeta = np.asfortranarray(vol)
    ne = grid.n_edges
    e0 = rng.standard_normal(ne) + (1j * rng.standard_normal(ne) if dtype is complex else 0)
    s0 = rng.standard_normal(ne) + (1j * rng.standard_normal(ne) if dtype is complex else 0)
    try:
        for name in SMOOTHERS:
            for nu in (2, 3, 4):
                out = []
                for skip in (1, 0):
                    lib.emg3d_set_option(b'skip_repeat', skip)
                    e = mg_ref.Field(grid, e0.astype(dtype).copy())
                    sf = mg_ref.Field(grid, s0.astype(dtype).copy())
                    getattr(core, name)(e.fx, e.fy, e.fz, sf.fx, sf.fy, sf.fz, eta[0], eta[1], eta[2], zeta,
                                        h[0], h[1], h[2], nu)
                    out.append(e.field.copy())
                assert np.array_equal(out[0], out[1]), (name, nu)
    finally:
        lib.emg3d_set_option(b'skip_repeat', 1)


@pytest.mark.parametrize('dtype', [complex, float])
def test_tiled_point_smoother_fused_sweeps(dtype):
    """Tiled point smoother: the tiles where two consecutive sweeps meet run both sweeps on one LDS
    copy (option tile_fuse), minus the repeated node colour (skip_repeat): identical bits with
    every combination of the two options, nu = 1..4, on a grid with partial tiles."""
    lib = _lib.lib()
    rng = np.random.default_rng(3)
    shape = (40, 11, 15)
    h = [widths(s - 4, 2, 30. + 7 * d, 1.2) for d, s in enumerate(shape)]
    grid = mg_ref.Grid(h, (0., 0., 0.))
    sval = 2j * np.pi * 0.7 if dtype is complex else -2.1
    vol = (h[0][:, None, None] * h[1][None, :, None] * h[2][None, None, :])
    eta = [np.asfortranarray(-sval * 1.25663706127e-06 * vol * 10 ** rng.uniform(-1, 1, shape)).astype(dtype)
           for _ in range(3)]
    zeta = np.asfortranarray(vol)
    ne = grid.n_edges
    e0 = rng.standard_normal(ne) + (1j * rng.standard_normal(ne) if dtype is complex else 0)
    s0 = rng.standard_normal(ne) + (1j * rng.standard_normal(ne) if dtype is complex else 0)
    old = lib.emg3d_get_option(b'point_tile_min')
    try:
        lib.emg3d_set_option(b'point_tile_min', 1)
        for nu in (1, 2, 3, 4):
            out = []
            for fuse, skip in ((1, 1), (1, 0), (0, 1), (0, 0)):
                lib.emg3d_set_option(b'tile_fuse', fuse)
                lib.emg3d_set_option(b'skip_repeat', skip)
                e = mg_ref.Field(grid, e0.astype(dtype).copy())
                sf = mg_ref.Field(grid, s0.astype(dtype).copy())
                core.gauss_seidel(e.fx, e.fy, e.fz, sf.fx, sf.fy, sf.fz, eta[0], eta[1], eta[2], zeta,
                                  h[0], h[1], h[2], nu)
                out.append(e.field.copy())
            for o in out[1:]:
                assert np.array_equal(out[0], o), nu
    finally:
        lib.emg3d_set_option(b'point_tile_min', old)
        lib.emg3d_set_option(b'tile_fuse', 1)
        lib.emg3d_set_option(b'skip_repeat', 1)


# ------------------------------------------------------------------------------------------
# Full-size per-sweep parity: the kernel instantiations bench.py times -- default options, so
# the partial-LDS (VMODE 2) and global-scratch (VMODE 0) record modes of k_line_colour and the
# un-forced tiled point path with fused sweeps are the ones executing -- against the oracle in
# the same ordering (order 1: four colours; order 2: tile-blocked point order).
# ------------------------------------------------------------------------------------------
def _host_fields(lv, grid, seed):
    s = _rand_field(lv, grid, seed, pec=False).cpu().numpy()
    e0 = _rand_field(lv, grid, seed + 1, pec=True).cpu().numpy()
    return s, e0


def _oracle_sweeps(fn, vm, grid, s, e0, nu, tiled):
    og = mg_ref.Grid(grid.h, grid.origin)
    S, A = mg_ref.Field(og, s), mg_ref.Field(og, e0.copy())
    order = 2 if (fn == 'gauss_seidel' and tiled) else 1
    getattr(ocore, fn)(A.fx, A.fy, A.fz, S.fx, S.fy, S.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta,
                       *grid.h, nu, order=order)
    return A.field


def _level_with_host_model(shape, case, seed, stretch=1.03, extras=False):
    """_rand_level, keeping the host arrays of the model for the oracle. extras: with epsilon_r (eta gets a
    real part a tenth of its imaginary one: eta = -s mu0 V (sigma + s eps0 eps_r), emg3d/models.py:677-691)
    and mu_r (zeta = V / mu_r)."""
    rng = np.random.default_rng(seed)
    h = [widths(n // 2, n // 4, 25., stretch) if n % 4 == 0 else
         25. * stretch ** np.abs(np.arange(n) - n // 2) for n in shape]
    grid = emg3d.TensorMesh(h, (0, 0, 0))
    assert grid.shape_cells == shape
    vol = grid.cell_volumes.reshape(shape, order='F')
    smu0 = 2j * np.pi * 1.0 * 1.25663706127e-06

    class VM:
        pass
    vm = VM()
    vm.grid, vm.case = grid, case
    sig = 10 ** rng.uniform(-1.5, 0.5, shape)
    vm.eta_x = np.asfortranarray(-smu0 * vol * sig)
    vm.eta_y = np.asfortranarray(vm.eta_x / 1.5) if case == 'triaxial' else vm.eta_x
    vm.eta_z = np.asfortranarray(vm.eta_x / 2.5) if case in ('VTI', 'triaxial') else vm.eta_x
    vm.zeta = np.asfortranarray(vol)
    if extras:
        disp = np.asfortranarray(-smu0 * vol * (0.1j * 10 ** rng.uniform(-1.5, 0.5, shape)))    # s eps0 eps_r: real eta
        vm.eta_x = vm.eta_x + disp
        vm.eta_y = vm.eta_y + disp if case == 'triaxial' else vm.eta_x
        vm.eta_z = vm.eta_z + disp if case in ('VTI', 'triaxial') else vm.eta_x
        vm.zeta = np.asfortranarray(vol / rng.uniform(0.7, 3.0, shape))
    lv = DeviceLevel.from_host(vm, torch.device('cuda'))
    assert bool(lv.flags & _lib.LEVEL_ETA_IMAG) == (not extras)
    return lv, grid, vm


@pytest.mark.parametrize('shape,case,extras', [((128, 128, 128), 'VTI', False), ((256, 256, 256), 'triaxial', False),
                                               ((128, 128, 128), 'VTI', True), ((160, 128, 96), 'triaxial', True)])
def test_full_size_per_sweep_parity_vs_oracle(shape, case, extras):
    """BASELINE.json configs 2 / 3 sizes, every smoother, nu = 2 (backward + forward sweep, the
    repeated colour pass skipped, the tiled point smoother with its fused sweeps), default
    library options: per-call values against the oracle in the same ordering, 2e-12 rel-L2. extras: the
    same with epsilon_r and mu_r -- eta with a real part, i.e. the tiled point smoother's full-width
    eta-sum layout (pst_stored_half false) at sizes that reach point_tile_min un-forced."""
    lv, grid, vm = _level_with_host_model(shape, case, 7, extras=extras)
    s, e0 = _host_fields(lv, grid, 11)
    lv.s.copy_(torch.from_numpy(s))
    nodes = (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)
    tiled = nodes >= _lib.lib().emg3d_get_option(b'point_tile_min') > 0
    assert tiled                                    # both sizes run the tiled point path
    for lr, fn in enumerate(SMOOTHERS):
        lv.e.copy_(torch.from_numpy(e0))
        lv.smooth(lr, 2)
        got = lv.e.cpu().numpy()
        want = _oracle_sweeps(fn, vm, grid, s, e0, 2, tiled)
        assert relerr(got, want) < 2e-12, (shape, fn)
        lv._factors.pop(lr, None)                   # free the 5 GB of line factors per direction
        torch.cuda.empty_cache()
    # the residual on the same level (at 256^3 a workgroup walks 8 planes, at 128^3 one) and its
    # norm, and the Krylov operator, against core.amat_x of the oracle
    og = mg_ref.Grid(grid.h, grid.origin)
    S, E = mg_ref.Field(og, s.copy()), mg_ref.Field(og, e0)
    ocore.amat_x(S.fx, S.fy, S.fz, E.fx, E.fy, E.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h)
    lv.e.copy_(torch.from_numpy(e0))
    norm = lv.residual(store=True, norm=True)
    assert relerr(lv.r.cpu().numpy(), S.field) < 1e-13
    assert norm == pytest.approx(np.linalg.norm(S.field), rel=1e-12)
    out = torch.empty_like(lv.e)
    lv.apply_A(lv.e, out)
    assert relerr(out.cpu().numpy(), s - S.field) < 1e-12          # A e = s - (s - A e)


@pytest.mark.parametrize('shape,lr', [
    ((128, 96, 96), 1), ((96, 128, 96), 2), ((96, 96, 130), 3),        # 16 lines / workgroup, partial-LDS records
    ((256, 96, 96), 1), ((96, 258, 96), 2), ((96, 96, 256), 3),        # records in the global scratch
    ((130, 6, 10), 1), ((6, 256, 10), 2), ((10, 6, 129), 3),           # long lines, few of them (4 lines / workgroup)
    ((384, 6, 10), 1), ((384, 96, 96), 1),                             # the x-lines of config 5 (384 x 256 x 256)
    ((60, 60, 384), 3),                                                # streamed kernel with 8 lines per workgroup
])
@pytest.mark.parametrize('dtype', [complex, float])
def test_long_line_record_modes_vs_oracle(shape, lr, dtype):
    """Line directions of 128 / 130 / 256 / 258 blocks: every record mode (VMODE 1 / 2 / 0) and
    lines-per-workgroup choice of the fused line kernel at the line lengths of the 128^3 and
    256^3 levels, at a size the oracle sweeps in a second; nu = 3, per call, 1e-11."""
    rng = np.random.default_rng(sum(shape) + lr)
    h = [rng.uniform(5., 15., n) * 1.02 ** np.abs(np.arange(n) - n // 2) for n in shape]
    grid = mg_ref.Grid(h, (0., 0., 0.))
    sig = [10 ** rng.uniform(-1, 1, shape) for _ in range(3)]
    vm = mg_ref.volume_model(grid, 0.7 if dtype is complex else -0.7, *sig)
    s, e0 = mg_ref.Field(grid, dtype=dtype), mg_ref.Field(grid, dtype=dtype)
    for f in (s, e0):
        f.field[:] = rng.standard_normal(f.field.size)
        if dtype is complex:
            f.field[:] += 1j * rng.standard_normal(f.field.size)
    for f in (e0.fx[:, 0, :], e0.fx[:, -1, :], e0.fx[:, :, 0], e0.fx[:, :, -1], e0.fy[0], e0.fy[-1],
              e0.fy[:, :, 0], e0.fy[:, :, -1], e0.fz[0], e0.fz[-1], e0.fz[:, 0], e0.fz[:, -1]):
        f[...] = 0
    fn = SMOOTHERS[lr]
    a, b = e0.copy(), e0.copy()
    args = (s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h, 3)
    getattr(ocore, fn)(a.fx, a.fy, a.fz, *args, order=1)
    getattr(core, fn)(b.fx, b.fy, b.fz, *args)
    # three sweeps of exact solves of lines of up to 258 blocks, eliminated from both ends
    # here and from one end in the oracle: round-off of the two orders, not of the sweep order
    assert relerr(b.field, a.field) < 1e-11, (shape, fn)


@pytest.mark.parametrize('kw,tile_min', [
    (dict(cycle='F', semicoarsening=True, linerelaxation=True), None),
    (dict(cycle='V', semicoarsening=False, linerelaxation=False), 1),
])
def test_solve_with_epsilon_r_and_mu_r_vs_oracle(kw, tile_min):
    """A whole solve on a model with epsilon_r AND mu_r (emg3d/models.py:677-691) at a frequency where the
    displacement current is comparable to the conduction current (eta gets a real part as large as its
    imaginary one; the level's ETA_IMAG flag is off): line smoothers on every level, and the tiled point
    smoother in its full-width eta-sum layout (point_tile_min = 1), against the oracle's driver in the same
    ordering -- same cycle count, converged fields to 1e-8."""
    lib = _lib.lib()
    shape = (40, 32, 24)
    rng = np.random.default_rng(17)
    # resistive rock (1-10 kOhm m), 1 m cells, 100 kHz: omega eps / sigma ~ 0.3, and the 50 m grid stays well
    # below the wavelength (~300 m) -- the operator is still diffusion-dominated and multigrid converges
    h = [widths(n // 2, n // 4, 1., 1.08) for n in shape]
    grid = emg3d.TensorMesh(h, [-w.sum() / 2 for w in h])
    assert grid.shape_cells == shape
    rho = 10 ** rng.uniform(3.0, 4.0, shape)
    eps = rng.uniform(1., 40., shape)
    mur = rng.uniform(0.8, 2.5, shape)
    freq = 1e5
    model = emg3d.Model(grid, rho, 1.5 * rho, 2.5 * rho, mu_r=mur, epsilon_r=eps)
    sfield = emg3d.get_source_field(grid, (0.5, -1., 0.25, 20., 30.), freq)
    ogrid = mg_ref.Grid(grid.h, grid.origin)
    vm = mg_ref.volume_model(ogrid, freq, 1 / rho, 1 / (1.5 * rho), 1 / (2.5 * rho), mu_r=mur, epsilon_r=eps)
    assert np.abs(vm.eta_x.real).max() > 0.05 * np.abs(vm.eta_x.imag).max()
    old = lib.emg3d_get_option(b'point_tile_min')
    try:
        if tile_min is not None:
            lib.emg3d_set_option(b'point_tile_min', tile_min)
        e, info = emg3d.solve(model, sfield, sslsolver=False, tol=1e-10, return_info=True, **kw)
    finally:
        lib.emg3d_set_option(b'point_tile_min', old)
    okw = dict(kw, order=1)
    if tile_min is not None:
        okw['tile_min'] = tile_min
    eo, io = mg_ref.solve(vm, mg_ref.Field(ogrid, sfield.field.copy()), tol=1e-10, **okw)
    assert info['exit'] == 0 and io['exit'] == 0, (info['exit_message'], io)
    assert info['it_mg'] == io['it_mg']
    assert relerr(e.field, eo.field) < 1e-8


@pytest.mark.slow
@pytest.mark.parametrize('name', ['marine128', 'triaxial256'])
def test_full_size_converged_vs_oracle_same_order(name):
    """BASELINE.json configs 2 and 3 at FULL size, exactly as bench.py builds them, solved to tol 1e-10 on the
    GPU and by the oracle's multigrid driver in the same smoother ordering (its independent classes walked
    by threads: bit-identical with the serial walk, tests/test_kernel_bodies_cpu.py): identical cycle
    counts, identical exit state, converged fields within 1e-10 rel-L2. (Round 3 ran this from
    tools/full_size_converged.py: 10 / 21 cycles, 1.6e-14 / 4.4e-13; oracle time ~15 s / ~4.5 min on 16
    threads.) The reference's sequential order reaches the same fixed point; it is compared on the reduced
    copies (test_bench_workloads_converged_vs_oracle) and at 32^3 against the reference itself."""
    from bench import workload
    wl = workload(name)
    grid = emg3d.TensorMesh(wl['h'], wl['origin'])
    model = emg3d.Model(grid, **wl['res'])
    sfield = emg3d.get_source_field(grid, wl['source'], wl['frequency'])
    e, info = emg3d.solve(model, sfield, sslsolver=False, tol=1e-10, return_info=True, **wl['opts'])
    field = e.field.copy()
    del e, model
    torch.cuda.empty_cache()
    ogrid = mg_ref.Grid(grid.h, grid.origin)
    cond = {k: 1.0 / np.asarray(v, dtype=float) for k, v in wl['res'].items()}
    vm = mg_ref.volume_model(ogrid, wl['frequency'], cond['property_x'], cond.get('property_y'), cond.get('property_z'))
    eo, io = mg_ref.solve(vm, mg_ref.Field(ogrid, sfield.field.copy()), tol=1e-10, order=1, **wl['opts'])
    assert info['exit'] == io['exit'] == 0, (info['exit_message'], io)
    assert info['it_mg'] == io['it_mg']
    assert info['rel_error'] == pytest.approx(io['rel_error'], rel=1e-3)
    assert relerr(field, eo.field) < 1e-10


@pytest.mark.parametrize('compact', [False, 'auto'])
def test_marine128_one_cycle_vs_oracle_same_order(compact):
    """BASELINE.json config 2 itself (bench.py workload 'marine128'): ONE F-cycle with
    semicoarsening and line relaxation on the GPU against the oracle's multigrid driver run in the
    same smoother ordering -- every level, transfer and smoother call of the cycle the bench
    times; with fp64 line records fields after the cycle agree to 1e-10 and the residual norms to 1e-9, with the
    default ('auto': compact records on the 128-block lines of level 0) to eps32 x cond of the blocks."""
    _one_cycle_vs_oracle('marine128', compact=compact)


@pytest.mark.parametrize('name', ['salt96', 'triaxial64'])
def test_bench_workloads_converged_vs_oracle(name):
    """Reduced copies of BASELINE.json configs 5 (salt-like, isotropic, F-cycle + sc + lr) and 3
    (tri-axial blocky model, W-cycle + sc + lr), exactly as bench.py builds them: converged GPU
    field vs the oracle in the reference's lexicographic order, both at tol 1e-10 -> 1e-8."""
    from bench import workload
    wl = workload(name)
    grid = emg3d.TensorMesh(wl['h'], wl['origin'])
    model = emg3d.Model(grid, **wl['res'])
    sfield = emg3d.get_source_field(grid, wl['source'], wl['frequency'])
    e, info = emg3d.solve(model, sfield, sslsolver=False, tol=1e-10, return_info=True, **wl['opts'])
    assert info['exit'] == 0, info['exit_message']
    ogrid = mg_ref.Grid(grid.h, grid.origin)
    cond = {k: 1.0 / np.asarray(v, dtype=float) for k, v in wl['res'].items()}
    vm = mg_ref.volume_model(ogrid, wl['frequency'], cond['property_x'], cond.get('property_y'),
                             cond.get('property_z'))
    eo, io = mg_ref.solve(vm, mg_ref.Field(ogrid, sfield.field.copy()), tol=1e-10, **wl['opts'])
    assert io['exit'] == 0
    assert relerr(e.field, eo.field) < 1e-8
    # the four-colour line ordering needs more cycles than the lexicographic one on this kind of model:
    # 1.25 x with the cyclic pass sequence of round 3 (triaxial64, W-cycle: 21-22 against 17 at tol 1e-10),
    # 1.5 x with the mirrored sweeps of rounds 1-2 -- the bound separates the two
    assert info['it_mg'] <= int(np.ceil(1.3 * io['it_mg']))


def _one_cycle_vs_oracle(name, source_index=0, compact=False):
    """ONE multigrid cycle of a bench workload, exactly as bench.py builds it, on the GPU and with the
    oracle's driver in the same smoother ordering: every level, transfer and smoother call (through
    the captured-graph path's eager first occurrence) of the cycle the bench times. compact = False: fp64 line
    records, the per-cycle tolerance 1e-10; 'auto' (the solver's default: single-precision T and w records on the
    levels that stream them, finest level in residual form): the same cycle with perturbed line solves -- equal to
    eps32 x cond of the blocks (1e-5 here), the residual norm after the cycle to 1e-3."""
    from bench import workload
    wl = workload(name, source_index=source_index)
    grid = emg3d.TensorMesh(wl['h'], wl['origin'])
    model = emg3d.Model(grid, **wl['res'])
    sfield = emg3d.get_source_field(grid, wl['source'], wl['frequency'])
    e, info = emg3d.solve(model, sfield, sslsolver=False, tol=1e-30, maxit=1, return_info=True, line_compact=compact,
                          **wl['opts'])
    assert info['it_mg'] == 1
    ogrid = mg_ref.Grid(grid.h, grid.origin)
    cond = {k: 1.0 / np.asarray(v, dtype=float) for k, v in wl['res'].items()}
    vm = mg_ref.volume_model(ogrid, wl['frequency'], cond['property_x'], cond.get('property_y'), cond.get('property_z'))
    eo, io = mg_ref.solve(vm, mg_ref.Field(ogrid, sfield.field.copy()), tol=1e-30, maxit=1, order=1, **wl['opts'])
    assert io['it_mg'] == 1
    if compact:
        assert info['residual_form'] is True
        assert 1e-12 < relerr(e.field, eo.field) < 1e-4
        assert info['abs_error'] == pytest.approx(io['abs_error'], rel=1e-2)
    else:
        assert relerr(e.field, eo.field) < 1e-10
        assert info['abs_error'] == pytest.approx(io['abs_error'], rel=1e-9)
    assert info['smoother_cell_sweeps'] == io['smooth_work']


@pytest.mark.slow
def test_triaxial256_one_cycle_vs_oracle_same_order():
    """BASELINE.json config 3 at full size -- the workload `bench.py` times by default: one W-cycle
    with semicoarsening and line relaxation (every semicoarsened level down to 256 x 2 x 2) against the
    oracle in the same ordering; ~1.5 min of oracle time."""
    _one_cycle_vs_oracle('triaxial256')


@pytest.mark.slow
def test_salt384_one_cycle_vs_oracle_same_order():
    """BASELINE.json config 5 at its real shape (384 x 256 x 256: 384-block x-lines), pair 7 (2 Hz,
    the source at x = +2000 m): one F-cycle against the oracle in the same ordering."""
    _one_cycle_vs_oracle('salt384', source_index=7)


@pytest.mark.slow
def test_salt384_pair0_one_cycle_vs_oracle_same_order():
    """Config 5's longest pair at full size -- pair 0 (0.25 Hz, the source at x = -2000 m: 9 cycles to 1e-6, 22 to
    1e-10) --: one F-cycle against the oracle in the same ordering, next to pair 7 above. (The pair converged to
    1e-10 against the oracle costs 5.5 min of oracle time on 16 threads, which the suite's time limit does not
    hold beside the converged configs 2 and 3 and pair 7 below; builder-run: tools/full_size_converged.py salt384:0 ->
    profiles/r06_full_size_converged.txt.)"""
    _one_cycle_vs_oracle('salt384', source_index=0)


@pytest.mark.slow
def test_salt384_pair7_converged_vs_oracle_same_order():
    """BASELINE.json config 5 at FULL size (384 x 256 x 256), its cheapest pair -- pair 7: 2 Hz, the source at
    x = +2000 m -- solved to tol 1e-10 with the solver's defaults (compact line records on the 384- and 256-block
    lines, finest level in residual form) and by the oracle's driver in the same smoother ordering (fp64 throughout):
    same cycle count, same exit state, converged fields within 1e-8 (BASELINE.json's tolerance; measured ~1e-12).
    The longest pair (pair 0, 0.25 Hz: 22 cycles, ~5.5 min of oracle time) is builder-run with the same code:
    tools/full_size_converged.py -> profiles/r06_full_size_converged.txt."""
    from bench import workload
    wl = workload('salt384', source_index=7)
    grid = emg3d.TensorMesh(wl['h'], wl['origin'])
    model = emg3d.Model(grid, **wl['res'])
    sfield = emg3d.get_source_field(grid, wl['source'], wl['frequency'])
    e, info = emg3d.solve(model, sfield, sslsolver=False, tol=1e-10, return_info=True, **wl['opts'])
    field = e.field.copy()
    del e, model
    torch.cuda.empty_cache()
    ogrid = mg_ref.Grid(grid.h, grid.origin)
    cond = {k: 1.0 / np.asarray(v, dtype=float) for k, v in wl['res'].items()}
    vm = mg_ref.volume_model(ogrid, wl['frequency'], cond['property_x'], cond.get('property_y'), cond.get('property_z'))
    eo, io = mg_ref.solve(vm, mg_ref.Field(ogrid, sfield.field.copy()), tol=1e-10, order=1, **wl['opts'])
    assert info['exit'] == io['exit'] == 0, (info['exit_message'], io)
    assert info['it_mg'] == io['it_mg']
    assert info['rel_error'] == pytest.approx(io['rel_error'], rel=1e-2)
    assert relerr(field, eo.field) < 1e-8


@pytest.mark.parametrize('pair', [3, 5, 6])
def test_salt96_other_pairs_converged_vs_oracle(pair):
    """Config 5's other (source, frequency) pairs on the quarter-size copy (pair 0 is in
    test_bench_workloads_converged_vs_oracle): 0.5 Hz / x = +2000 m, 1 Hz / +2000 m, 2 Hz / -2000 m
    -- with pair 0, all four frequencies and both sources; converged against the lexicographic
    oracle at 1e-8."""
    from bench import workload
    wl = workload('salt96', source_index=pair)
    grid = emg3d.TensorMesh(wl['h'], wl['origin'])
    model = emg3d.Model(grid, **wl['res'])
    sfield = emg3d.get_source_field(grid, wl['source'], wl['frequency'])
    e, info = emg3d.solve(model, sfield, sslsolver=False, tol=1e-10, return_info=True, **wl['opts'])
    assert info['exit'] == 0, info['exit_message']
    ogrid = mg_ref.Grid(grid.h, grid.origin)
    vm = mg_ref.volume_model(ogrid, wl['frequency'], 1.0 / wl['res']['property_x'])
    eo, io = mg_ref.solve(vm, mg_ref.Field(ogrid, sfield.field.copy()), tol=1e-10, **wl['opts'])
    assert io['exit'] == 0
    assert relerr(e.field, eo.field) < 1e-8
    assert info['it_mg'] <= int(np.ceil(1.3 * io['it_mg']))


@pytest.mark.slow
def test_config4_eight_sources_batch_equals_separate_and_oracle():
    """BASELINE.json config 4 on one GPU: the 8 sources of the 128^3 marine model solved together
    (solve_batch) give bit for bit the fields, cycle counts and error histories of 8 separate
    solves; source 7 (x = +1400 m, the one farthest from the single-source bench workload) agrees
    with the oracle's converged field (lexicographic order, both at tol 1e-9) to 1e-8."""
    from bench import workload
    wls = [workload('marine128', source_index=i) for i in range(8)]
    grid = emg3d.TensorMesh(wls[0]['h'], wls[0]['origin'])
    model = emg3d.Model(grid, **wls[0]['res'])
    opts = dict(wls[0]['opts'], tol=1e-9)
    sfields = [emg3d.get_source_field(grid, w['source'], w['frequency']) for w in wls]
    assert len({w['source'] for w in wls}) == 8
    hier = solver.Hierarchy(emg3d.models.VolumeModel(model, sfields[0]))
    sep = [emg3d.solve(model, sf, sslsolver=False, return_info=True, hierarchy=hier, **opts) for sf in sfields]
    del hier
    torch.cuda.empty_cache()
    bat = emg3d.solve_batch(model, sfields, **opts)
    for (e1, i1), (e2, i2) in zip(sep, bat):
        assert i1['exit'] == i2['exit'] == 0 and i1['it_mg'] == i2['it_mg']
        assert np.array_equal(i1['error_at_cycle'], i2['error_at_cycle'])
        assert np.array_equal(e1.field, e2.field)
    ogrid = mg_ref.Grid(grid.h, grid.origin)
    cond = {k: 1.0 / np.asarray(v, dtype=float) for k, v in wls[7]['res'].items()}
    vm = mg_ref.volume_model(ogrid, 1.0, cond['property_x'], None, cond['property_z'])
    eo, io = mg_ref.solve(vm, mg_ref.Field(ogrid, sfields[7].field.copy()), **opts)
    assert io['exit'] == 0
    assert relerr(sep[7][0].field, eo.field) < 1e-8


@pytest.mark.parametrize('kw', [dict(cycle='W', semicoarsening=True, linerelaxation=True),
                                dict(cycle='F', semicoarsening=False, linerelaxation=7),
                                dict(cycle='V', semicoarsening=True, linerelaxation=2, sslsolver=True)])
def test_line_factor_policy_rebuild_equals_resident(kw):
    """Hierarchy(line_factors='rebuild' / 'single'): two / one factor buffers per level, re-factorised when the line-relaxation
    code asks for a direction neither holds (the finest level from cycle to cycle, coarse levels inside every
    coarse-grid correction, also when that correction is replayed from a captured graph: > 3 occurrences of
    every variant here). Same factors, same kernels: fields, cycle counts and error histories bit-identical to
    the resident policy; the line-factor bytes of the hierarchy drop to at most 2/3."""
    shape = (32, 24, 40)
    rng = np.random.default_rng(3)
    h = [widths(n // 2, n // 4, 30., 1.1) for n in shape]
    grid = emg3d.TensorMesh(h, [-w.sum() / 2 for w in h])
    rho = 10 ** rng.uniform(-0.5, 1.0, shape)
    model = emg3d.Model(grid, rho, 1.5 * rho, 2.5 * rho)
    sfield = emg3d.get_source_field(grid, (3., -2., 1., 20., 30.), 0.8)
    opts = dict({'sslsolver': False, 'tol': 1e-11, 'maxit': 40}, **kw)
    vmodel = emg3d.models.VolumeModel(model, sfield)
    out, nbytes = {}, {}

    def factor_bytes(lv, seen):
        if id(lv) in seen:
            return 0
        seen.add(id(lv))
        n = sum(f.numel() + lf.numel() for k, (f, lf) in lv._factors.items() if k in (1, 2, 3))
        n += sum(sl['fac'].numel() + sl['lfac'].numel() for sl in lv.__dict__.get('_slots', []))
        return n + sum(factor_bytes(link['level'], seen) for link in lv.children.values())
    for policy in ('resident', 'rebuild', 'single'):
        hier = solver.Hierarchy(vmodel, line_factors=policy)
        e, info = emg3d.solve(model, sfield, return_info=True, hierarchy=hier, **opts)
        e2, info2 = emg3d.solve(model, sfield, return_info=True, hierarchy=hier, **opts)     # reused: graphs replayed from the start
        assert np.array_equal(e.field, e2.field) and info['it_mg'] == info2['it_mg']
        out[policy] = (e.field.copy(), info)
        nbytes[policy] = factor_bytes(hier.top, set())
        if policy != 'resident' and kw['linerelaxation'] in (True, 7):
            assert hier.top.factor_rebuilds >= 3
        del hier
    e1, i1 = out['resident']
    for policy in ('rebuild', 'single'):
        e2, i2 = out[policy]
        assert i1['exit'] == i2['exit'] and i1['it_mg'] == i2['it_mg'] and i1['it_mg'] >= 6
        assert np.array_equal(i1['error_at_cycle'], i2['error_at_cycle'])
        assert np.array_equal(e1, e2)
    if kw['linerelaxation'] in (True, 7):
        # (two / one buffer per level, each sized for the level's largest direction: on the slab-shaped levels of
        # a semicoarsened hierarchy the padded records of short lines cost more than a third)
        # (the buffers of 'rebuild' / 'single' are sized for a level's largest direction -- with compact records on some
        #  directions and fp64 + N records on others the saving against 'resident' is smaller than 1/3 / 2/3)
        assert nbytes['single'] < nbytes['rebuild'] < nbytes['resident'] and nbytes['single'] <= 0.6 * nbytes['resident'], nbytes
    with pytest.raises(ValueError, match='line_factors'):
        solver.Hierarchy(vmodel, line_factors='sometimes')


@pytest.mark.slow
def test_512_cubed_w_cycle_with_rebuilt_line_factors():
    """512^3 (134 M cells, 403 M unknowns) on ONE GPU: the tri-axial workload of config 3 at twice its edge length,
    W-cycle with semicoarsening and line relaxation, hierarchy policy 'rebuild' (two line-factor buffers per level:
    233 GB for the whole hierarchy against 274 GB with every direction resident). One cycle reduces the error
    by more than an order of magnitude (tools/big_cube.py compared this very cycle with the oracle in the same
    ordering: 1.1e-12 rel-L2, profiles/r04_big_cube.txt), and the operator on the finest level keeps the
    size-independent properties of test_full_size_operator_properties: linear, complex symmetric, residual(0) = s."""
    from bench import workload
    if torch.cuda.get_device_properties(0).total_memory < 250e9:
        pytest.skip('needs the 288 GB of an MI355X')
    wl = workload('triaxial512')
    grid = emg3d.TensorMesh(wl['h'], wl['origin'])
    assert grid.shape_cells == (512, 512, 512)
    model = emg3d.Model(grid, **wl['res'])
    sfield = emg3d.get_source_field(grid, wl['source'], wl['frequency'])
    hier = solver.Hierarchy(emg3d.models.VolumeModel(model, sfield), line_factors='rebuild')
    _, info = emg3d.solve(model, sfield, sslsolver=False, tol=1e-30, maxit=1, return_info=True, hierarchy=hier,
                          _download=False, **wl['opts'])
    assert info['it_mg'] == 1 and np.isfinite(info['rel_error']) and info['rel_error'] < 0.05
    assert hier.top.factor_rebuilds == 2 and len(hier.top._slots) == 2
    assert torch.cuda.max_memory_allocated() < 200e9
    lv = hier.top
    x, y = _rand_field(lv, grid, 2), _rand_field(lv, grid, 3)
    lv.s.zero_()

    def A(v):
        lv.e.copy_(v)
        lv.residual(store=True, norm=False)
        return -lv.r.clone()
    ax, ay = A(x), A(y)
    a, b = 0.7 - 0.2j, -1.3 + 0.5j
    lin = A(a * x + b * y)
    assert (torch.linalg.norm(lin - (a * ax + b * ay)) / torch.linalg.norm(lin)).item() < 1e-13
    xay, yax = torch.sum(x * ay).item(), torch.sum(y * ax).item()
    assert abs(xay - yax) / abs(xay) < 1e-11
    lv.s.copy_(x)
    lv.e.zero_()
    n = lv.residual(store=True, norm=True)
    assert torch.equal(lv.r, x)
    assert n == pytest.approx(torch.linalg.norm(x).item(), rel=1e-13)
    del hier, lv, x, y, ax, ay, lin
    torch.cuda.empty_cache()


def test_hierarchy_field_follows_a_solve_that_has_nothing_to_do():
    """A solve that takes the zero-source / already-converged shortcut on a reused hierarchy must
    leave THIS solve's field in HBM (receivers and the gradient read it there), not the previous
    pair's; and a pair without data contributes nothing to the gradient."""
    from emg3d_amd import gradient
    hx = widths(8, 2, 50., 1.3)
    grid = emg3d.TensorMesh([hx, hx, hx], (-hx.sum() / 2,) * 3)
    model = emg3d.Model(grid, 1.0)
    sfield = emg3d.get_source_field(grid, (0., 0., 0., 0., 0.), 1.0)
    hier = solver.Hierarchy(emg3d.models.VolumeModel(model, sfield))
    emg3d.solve(model, sfield, sslsolver=False, hierarchy=hier)
    assert float(hier.top.e.abs().max()) > 0
    zero = emg3d.Field(grid, frequency=1.0)
    e0, info = emg3d.solve(model, zero, sslsolver=False, hierarchy=hier, return_info=True)
    assert info['exit'] == 0 and not np.any(e0.field)
    assert float(hier.top.e.abs().max()) == 0.0
    # gradient: one pair with data, one all-NaN pair
    rec = [(100., 50., 20., 0., 0.), (-120., 30., -40., 90., 0.)]
    sources = {'A': (0., 0., 0., 0., 0.), 'B': (60., -30., 10., 20., 0.)}
    freqs = {'f': 1.0}
    obs = {('A', 'f'): np.array([1e-11 + 2e-11j, -3e-11j]), ('B', 'f'): np.array([np.nan, np.nan])}
    m2, g2, i2 = gradient.misfit_and_gradient(model, sources, freqs, rec, obs, solver_opts={'tol': 1e-8})
    m1, g1, _ = gradient.misfit_and_gradient(model, {'A': sources['A']}, freqs, rec, {('A', 'f'): obs[('A', 'f')]},
                                            solver_opts={'tol': 1e-8})
    assert i2[('B', 'f')]['backward'] is None
    assert m2 == pytest.approx(m1, rel=1e-12) and np.array_equal(g1, g2)


def test_failed_krylov_leaves_a_provided_start_field_alone():
    """A diverging / stagnating preconditioner aborts the Krylov solver: the zero field solve() made
    itself comes back as zeros, a start field the caller provided is not overwritten
    (emg3d/solver.py:764-770: SciPy works on a copy, the assignment never happens)."""
    hx = widths(8, 2, 50., 1.3)
    grid = emg3d.TensorMesh([hx, hx, hx], (-hx.sum() / 2,) * 3)
    model = emg3d.Model(grid, 1.0)
    sfield = emg3d.get_source_field(grid, (0., 0., 0., 0., 0.), 1.0)
    rng = np.random.default_rng(3)
    start = emg3d.Field(grid, frequency=1.0)
    start.field[:] = 1e-9 * (rng.standard_normal(start.field.size) + 1j * rng.standard_normal(start.field.size))
    # gcrotmk preconditions unit-norm vectors: the multigrid's divergence rule aborts the first call
    # (the first call also zeroes the PEC faces of the start field, emg3d/solver.py:349-355)
    for attempt in range(2):
        before = start.field.copy()
        info = emg3d.solve(model, sfield, efield=start, sslsolver='gcrotmk', return_info=True)
        assert info['exit'] == 1 and 'returned field is zero' in info['exit_message']
        assert np.any(start.field)
    assert np.array_equal(start.field, before)
    e, info = emg3d.solve(model, sfield, sslsolver='gcrotmk', return_info=True)
    assert info['exit'] == 1 and not np.any(e.field)


# every method and dtype on 24 x 16 x 20 cells, and BiCGSTAB on 64 x 56 x 52: 578 924 edges, more than the 524 288 entries
# that one trip of the Krylov kernels' capped grid covers (csrc/krylov.h: 2048 workgroups of 256)
_KRYLOV_CASES = [pytest.param(method, dtype, (24, 16, 20), id=f'{dtype.__name__}-{method}') for dtype in (complex, float)
                 for method in ('bicgstab', 'cgs', 'gcrotmk', 'gcrotmk(1,1)')]
_KRYLOV_CASES.append(pytest.param('bicgstab', complex, (64, 56, 52), id='complex-bicgstab-64x56x52'))


@pytest.mark.parametrize('method, dtype, shape', _KRYLOV_CASES)
def test_device_krylov_matches_scipy_iteration(method, dtype, shape, monkeypatch):
    """The device BiCGSTAB / CGS / GCROT(m,k) (csrc/krylov.h: fused updates + inner products, scalars
    in a device table) against scipy.sparse.linalg's own iteration driven with the same device operator and
    multigrid preconditioner through host vectors: same status, same number of iterations and
    multigrid cycles, same true-residual history (1e-6 relative), fields equal to 1e-9."""
    import functools
    import scipy.sparse.linalg as ssl
    from emg3d_amd import models as emodels
    from emg3d_amd import _krylov
    sopts = {}
    if method == 'gcrotmk(1,1)':
        # short inner cycles: several outer iterations, recycled (c, u) pairs, the oldest one dropped
        method, sopts = 'gcrotmk', dict(m=1, k=1)
        monkeypatch.setattr(_krylov, 'gcrotmk', functools.partial(_krylov.gcrotmk, **sopts))
    rng = np.random.default_rng(5)
    h = [widths(n // 2, n // 4, 20., 1.2) for n in shape]
    grid = emg3d.TensorMesh(h, [-w.sum() / 2 for w in h])
    rho = 10 ** rng.uniform(-0.5, 1.0, shape)
    model = emg3d.Model(grid, rho, 1.5 * rho, 2.0 * rho)
    freq = 1.2 if dtype is complex else -1.2
    sfield = emg3d.get_source_field(grid, (3., -2., 1., 20., 30.), freq)
    if method == 'gcrotmk':
        # GCROT preconditions vectors of norm 1; the multigrid's divergence rule measures them against
        # the norm of the SOURCE (emg3d/solver.py:1627) -- with a unit dipole's 1e-9 the reference
        # aborts its first preconditioner call as DIVERGED (and so does this solver: see
        # test_krylov_with_multigrid_preconditioner). A source of norm 100 lets the iteration run.
        sfield.field *= 100 / np.linalg.norm(sfield.field)
    kw = dict(sslsolver=method, cycle='F', semicoarsening=True, linerelaxation=True, tol=1e-10 if sopts else 1e-8, maxit=30)
    e, info = emg3d.solve(model, sfield, return_info=True, **kw)
    assert info['exit'] == 0, info['exit_message']

    # SciPy's iteration on host vectors, device operator and preconditioner
    var = solver.MGParameters(verb=0, shape_cells=shape, **kw)
    var.l2_refe = float(np.linalg.norm(sfield.field))
    var.error_at_cycle[0] = var.l2_refe
    vm = emodels.VolumeModel(model, sfield)
    hier = solver.Hierarchy(vm)
    top = hier.top
    dt = sfield.field.dtype

    def up(v):
        return torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).cuda()

    def amat(v):
        return top.apply_A(up(v), torch.empty_like(top.e)).cpu().numpy()

    def prec(v):
        top.s.copy_(up(v))
        top.e.zero_()
        solver._multigrid(top, var, 0, 0)
        return top.e.cpu().numpy()
    n = sfield.field.size
    hist = []

    def cb(x):
        top.s.copy_(up(sfield.field))
        top.e.copy_(up(x))
        hist.append(top.residual(store=False, norm=True))
        solver._krylov_callback(var, hist[-1])
    x, code = getattr(ssl, method)(ssl.LinearOperator((n, n), matvec=amat, dtype=dt), sfield.field, x0=np.zeros(n, dt),
                                   rtol=var.tol, atol=1e-30, maxiter=var.ssl_maxit,
                                   M=ssl.LinearOperator((n, n), matvec=prec, dtype=dt), callback=cb, **sopts)
    assert code == 0
    if sopts:
        assert len(hist) >= 4          # (outer iterations: the recycling path is exercised)
    assert info['it_ssl'] == len(hist)
    assert info['it_mg'] == var.it
    assert np.allclose(info['error_at_cycle'], var.error_at_cycle, rtol=1e-6)      # multigrid cycles and Krylov steps
    assert relerr(e.field, x) < 1e-9


_TWO_RANK_COMPUTE = r"""
import os, sys, pickle
import numpy as np
import torch, torch.distributed as dist
root = os.environ['EMG3D_TEST_ROOT']
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, 'tests'))
import emg3d_amd as emg3d
from emg3d_amd import parallel
from helpers import widths
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
# the process group exists before the product's code runs (a launcher's job): collectives over gloo, every rank
# on the box's one GPU -- parallel.init() must join it as it is and still put the solves on cuda:0
torch.cuda.set_device(0)
dist.init_process_group('gloo', rank=rank, world_size=world)
hx = widths(8, 4, 50., 1.2)
grid = emg3d.TensorMesh([hx, hx[:12], hx], (-hx.sum() / 2, -330., -hx.sum() / 2))
model = None
if rank == 0:
    rng = np.random.default_rng(5)
    model = emg3d.Model(grid, 10 ** rng.uniform(-0.5, 0.5, grid.shape_cells), property_z=10 ** rng.uniform(0, 0.7, grid.shape_cells))
sources = {f'S{i}': (-160. + 70. * i, 20. * i - 30., 10., 15. * i, 0.) for i in range(5)}
freqs = {'f1': 1.0, 'f2': 3.0}
rng = np.random.default_rng(9)
rec = (rng.uniform(-150, 150, 6), rng.uniform(-100, 100, 6), rng.uniform(-100, 100, 6), 0., 0.)
opts = {'sslsolver': False, 'tol': 1e-8, 'verb': 0}
costs = [3., 1., 1., 1., 2., 2., 1., 1., 1., 1.]
out = parallel.compute(model, grid if rank == 0 else None, sources, freqs, opts, receivers=rec, costs=costs)
bat = parallel.compute(model, grid if rank == 0 else None, sources, freqs, opts, receivers=rec, costs=costs, batch=2,
                       keep_fields=False)
res = {'rank': rank, 'mine': sorted(k for k in out if k != '_all_info'),
       'fields': {k: out[k][0].field for k in out if k != '_all_info'},
       'responses': {k: out[k][1]['responses'] for k in out if k != '_all_info'},
       'it': {k: out[k][1]['it_mg'] for k in out if k != '_all_info'},
       'batched_responses': {k: bat[k][1]['responses'] for k in bat if k != '_all_info'},
       'all_info_keys': sorted(out['_all_info']) if rank == 0 else None,
       'all_responses': {k: v['responses'] for k, v in out['_all_info'].items()} if rank == 0 else None}
# what broadcast_model leaves behind on a rank that received the model: property arrays in HBM
m2 = parallel.broadcast_model(model, 0, torch.device('cuda', 0))
res['device_props'] = {n: (str(t.device), tuple(t.shape)) for n, t in m2.__dict__.get('_device_props', {}).items()}
res['prop_x_sum'] = float(np.sum(m2.property_x))
with open(os.path.join(os.environ['EMG3D_TEST_OUT'], f'rank{rank}.pkl'), 'wb') as f:
    pickle.dump(res, f)
parallel.finalize()
"""


def test_parallel_compute_two_ranks_real_solves_on_one_gpu(tmp_path):
    """parallel.compute with TWO ranks and real solves (the multi-GPU path short of RCCL: a gloo process group that
    exists before the product's code runs, both ranks on this box's one GPU): the model goes from rank 0 to rank 1
    through broadcast_model (property arrays stay in HBM there), the 10 pairs are shared out by longest-processing-
    time-first, every pair is solved exactly once, rank 0 gathers every pair's info and responses, and each field
    and response equals, bit for bit, what a single process computes for that pair; batched pairs (batch = 2)
    give the same responses."""
    import pickle
    import subprocess
    import sys
    from emg3d_amd import parallel
    script = tmp_path / 'two_ranks.py'
    script.write_text(_TWO_RANK_COMPUTE)
    env = dict(os.environ, EMG3D_TEST_ROOT=ROOT, EMG3D_TEST_OUT=str(tmp_path), HSA_ENABLE_IPC_MODE_LEGACY='0')
    import socket
    sk = socket.socket(); sk.bind(('127.0.0.1', 0)); port = sk.getsockname()[1]; sk.close()
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                        '--master-addr', '127.0.0.1', '--master-port', str(port), str(script)],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = [pickle.load(open(tmp_path / f'rank{k}.pkl', 'rb')) for k in (0, 1)]
    sources = {f'S{i}': (-160. + 70. * i, 20. * i - 30., 10., 15. * i, 0.) for i in range(5)}
    freqs = {'f1': 1.0, 'f2': 3.0}
    pairs = parallel.srcfreq_pairs(sources, freqs)
    costs = [3., 1., 1., 1., 2., 2., 1., 1., 1., 1.]
    for k in (0, 1):
        assert res[k]['mine'] == sorted(pairs[i] for i in parallel.shard(10, k, 2, costs))
        assert res[k]['device_props'] and all(d == 'cuda:0' for d, _ in res[k]['device_props'].values())
    assert res[0]['prop_x_sum'] == res[1]['prop_x_sum']
    assert sorted(res[0]['mine'] + res[1]['mine']) == sorted(pairs) == res[0]['all_info_keys']
    # the same pairs in this (single) process
    hx = widths(8, 4, 50., 1.2)
    grid = emg3d.TensorMesh([hx, hx[:12], hx], (-hx.sum() / 2, -330., -hx.sum() / 2))
    rng = np.random.default_rng(5)
    model = emg3d.Model(grid, 10 ** rng.uniform(-0.5, 0.5, grid.shape_cells), property_z=10 ** rng.uniform(0, 0.7, grid.shape_cells))
    rng = np.random.default_rng(9)
    rec = (rng.uniform(-150, 150, 6), rng.uniform(-100, 100, 6), rng.uniform(-100, 100, 6), 0., 0.)
    one = parallel.compute(model, grid, sources, freqs, {'sslsolver': False, 'tol': 1e-8, 'verb': 0}, receivers=rec)
    for k in (0, 1):
        for key in res[k]['mine']:
            assert np.array_equal(res[k]['fields'][key], one[key][0].field), (k, key)
            assert np.array_equal(res[k]['responses'][key], one[key][1]['responses'])
            assert np.array_equal(res[k]['batched_responses'][key], one[key][1]['responses'])
            assert res[k]['it'][key] == one[key][1]['it_mg']
            assert np.array_equal(res[0]['all_responses'][key], one[key][1]['responses'])


@pytest.mark.parametrize('backend', ['gloo', 'nccl'])
def test_bench_two_ranks_through_its_own_launcher(backend):
    """`python bench.py --gpus 2` as a driver would call it: bench.py spawns its two ranks itself
    (torch.distributed.run on 127.0.0.1). 'gloo': the ranks share this box's one GPU and run their
    collectives over gloo (EMG3D_BENCH_BACKEND); 'nccl' (needs two GPUs, skipped otherwise): one rank
    per GPU over RCCL, the property arrays broadcast device to device. Either way the product's
    multi-GPU path: parallel.init, parallel.broadcast_model (rank 1 never builds the model), rank-
    dependent source, barrier, MAX / SUM reductions and the rank-0 JSON line."""
    import json
    import subprocess
    import sys
    if backend == 'nccl' and torch.cuda.device_count() < 2:
        pytest.skip("RCCL leg needs two GPUs on the box")
    env = dict(os.environ, EMG3D_BENCH_BACKEND=backend, HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--workload', 'marine64',
                        '--steps', '3', '--warmup', '1', '--no-256', '--no-survey', '--no-cpu-baseline'],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['steps'] == 3 and out['scaling'] == 'weak'
    assert out['config']['workload'] == 'marine64' and out['value'] > 0
    assert out['config']['broadcast_ms'] > 0 and backend in out['config']['model_distribution']
    # two independent sources: twice the cell-sweeps of one rank per step
    assert out['config']['cell_sweeps_per_step'] > 0
    assert out['value'] == pytest.approx(2 * out['config']['cell_sweeps_per_step'] * 3 / (out['ms_per_step'] * 3e-3) / 1e6, rel=0.02)


def test_bench_plain_run_dumps_the_field_of_its_timed_cycles(tmp_path):
    """`python bench.py --steps K --dump-outputs DIR` without --full: K timed cycles, `ms_per_step`, none of the
    blocks of --full, and the field after the last timed cycle in DIR -- the same field a solver.multigrid call
    with as many cycles from the same start leaves (the bench's preparation + warm-up + timed cycles)."""
    import json
    import subprocess
    import sys
    import bench
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--workload', 'triaxial64', '--steps', '3',
                        '--warmup', '1', '--dump-outputs', str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['steps'] == 3 and out['warmup'] == 1 and out['ms_per_step'] > 0 and out['value'] > 0
    assert out['value'] == pytest.approx(out['config']['cell_sweeps_per_step'] / (out['ms_per_step'] * 1e-3) / 1e6, rel=1e-9)
    assert out['cpu_baseline'] is None
    assert not {'time_to_tol', 'fp64_storage', 'smoothers_256', 'survey_8_sources', 'survey_config5'} & set(out)
    re_, im_ = np.load(tmp_path / 'efield_real.npy'), np.load(tmp_path / 'efield_imag.npy')
    assert re_.dtype == im_.dtype == np.float64
    # the same cycles in this process: the bench's hierarchy and cycle driver, as many cycles as the bench ran
    wl = bench.workload('triaxial64')
    grid = emg3d.TensorMesh(wl['h'], wl['origin'])
    b = bench.Bench(wl, emg3d.Model(grid, **wl['res']), torch.device('cuda', 0))
    b.cycles((b.solver._GRAPH_AFTER + 1) * b.var.maxcycle)
    b.cycles(1)
    b.cycles(3)
    e = b.hier.top.solution().cpu().numpy()
    assert re_.size == grid.n_edges <= bench.DUMP_SAMPLE
    assert relerr(re_ + 1j * im_, e) < 1e-12


@pytest.mark.slow
@pytest.mark.parametrize('wlname', ['marine128', 'salt384'])
def test_bench_eight_ranks_dry_run_on_one_gpu(wlname):
    """`python bench.py --gpus 8 --workload marine128` (and `salt384`: config 5, eight (source, frequency) pairs shared
    out longest-first, 8 x ~24 GB of hierarchies on the one GPU) -- BASELINE.json configs 4 / 5 at their real rank count -- as the
    driver's scaling run calls it, with the eight ranks sharing this box's one GPU and their collectives over gloo
    (EMG3D_BENCH_BACKEND): process-group setup, the model broadcast to seven receiving ranks, one source per rank,
    barrier, MAX / SUM reductions, the rank-0 JSON line. So that the first 8-GPU run is not the first execution of
    this path. (Eight 128^3 hierarchies are 8 x 4.2 GB of the one GPU's HBM.)"""
    import json
    import subprocess
    import sys
    env = dict(os.environ, EMG3D_BENCH_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '8', '--workload', wlname,
                        '--steps', '2', '--warmup', '1', '--no-256', '--no-survey', '--no-cpu-baseline'],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['n_gpus'] == 8 and out['steps'] == 2 and out['scaling'] == 'weak'
    assert out['config']['workload'] == wlname and out['value'] > 0
    assert out['config']['broadcast_ms'] > 0 and 'gloo' in out['config']['model_distribution']
    # the scalars a scaling run reads: rank count, slowest / fastest rank's clock, the broadcast
    assert out['broadcast_ms'] == out['config']['broadcast_ms'] and out['backend'] == 'gloo'
    assert 0 < out['ms_per_step_rank_min'] <= out['ms_per_step_rank_max'] == out['ms_per_step']
    # eight independent sources: the aggregate is the sum over the ranks
    assert out['value'] == pytest.approx(8 * out['config']['cell_sweeps_per_step'] * 2 / (out['ms_per_step'] * 2e-3) / 1e6, rel=0.02)


@pytest.mark.parametrize('name,cycles', [('uni32_F', 10), ('marine32_W', 8)])
def test_32cubed_solves_vs_the_reference_itself(golden_solves32, name, cycles):
    """Converged fields of the reference (imported un-jitted in the build container,
    tools/make_golden.py solves32) at 32^3: BASELINE.json config 1 (plain F-cycle: the point
    smoother) and a stretched marine VTI model with W-cycle + semicoarsening + line relaxation.
    GPU at tol 1e-10: rel-L2 <= 1e-8 (the bar of BASELINE.json)."""
    g = golden_solves32
    p = name + '_'
    grid = emg3d.TensorMesh([g[p + 'hx'], g[p + 'hy'], g[p + 'hz']], g[p + 'origin'])
    kwm = {'property_x': g[p + 'res_x']}
    if p + 'res_z' in g.files:
        kwm['property_z'] = g[p + 'res_z']
    model = emg3d.Model(grid, **kwm)
    sfield = emg3d.get_source_field(grid, g[p + 'source'], float(g[p + 'frequency']))
    kw = {k[len(p) + 3:]: g[k].item() for k in g.files if k.startswith(p + 'kw_')}
    for k in ('semicoarsening', 'linerelaxation'):
        if isinstance(kw[k], (bool, np.bool_)):
            kw[k] = bool(kw[k])
    e, info = emg3d.solve(model, sfield, sslsolver=False, tol=1e-10, return_info=True, **kw)
    assert info['exit'] == 0, info['exit_message']
    assert relerr(e.field, g[p + 'efield']) < 1e-8
    assert int(g[p + 'tol1e-10_it_mg']) == cycles and abs(info['it_mg'] - cycles) <= 3
    if name == 'uni32_F':          # config 1 as stated: tol 1e-6
        _, i6 = emg3d.solve(model, sfield, sslsolver=False, tol=1e-6, return_info=True, **kw)
        assert i6['exit'] == 0 and abs(i6['it_mg'] - 6) <= 1


def test_gradient_kernel_and_adjoint_gradient_vs_reference(golden_gradient):
    """SURVEY.md 8f rank 4. (1) emg3d_dev_gradient_accumulate on the reference's forward and
    back-propagated fields against maps.interp_edges_to_vol_averages of real(b smu0 e) (1e-14);
    (2) gradient.misfit_and_gradient -- forward solve, linear responses, residual source,
    back-propagation, cell reduction, derivative chain -- against the misfit and gradient the
    reference's functions give for the same data (solves at tol 1e-9: 1e-5)."""
    from emg3d_amd import gradient
    from emg3d_amd._device import _ptr
    g = golden_gradient
    grid = emg3d.TensorMesh([g['hx'], g['hy'], g['hz']], g['origin'])
    nx, ny, nz = grid.shape_cells
    dev = torch.device('cuda')
    e, b = torch.from_numpy(g['efield']).to(dev), torch.from_numpy(g['bfield']).to(dev)
    vol = torch.from_numpy(np.ascontiguousarray(grid.cell_volumes)).to(dev)
    out = torch.zeros(3 * grid.n_cells, dtype=torch.float64, device=dev)
    smu0 = 2j * np.pi * float(g['frequency']) * float(g['meta_mu_0'])
    o1, o2, nc = grid.n_edges_x, grid.n_edges_x + grid.n_edges_y, grid.n_cells
    for _ in range(2):      # accumulates
        _lib.check(_lib.lib().emg3d_dev_gradient_accumulate(
            nx, ny, nz, 1, _ptr(e), _ptr(e, o1), _ptr(e, o2), _ptr(b), _ptr(b, o1), _ptr(b, o2), smu0.real, smu0.imag,
            _ptr(vol), _ptr(out), _ptr(out, nc), _ptr(out, 2 * nc), None), 'emg3d_dev_gradient_accumulate')
    got = out.cpu().numpy().reshape(3, nz, ny, nx).transpose(0, 3, 2, 1)
    assert relerr(got, 2 * g['grad_cells_raw']) < 1e-14

    model = emg3d.Model(grid, property_x=g['res_x'], property_z=g['res_z'])
    key = ('s1', 'f1')
    misfit, grad, info = gradient.misfit_and_gradient(
        model, {'s1': tuple(g['source'])}, {'f1': float(g['frequency'])}, g['receivers'], {key: g['observed']},
        {key: g['weights']}, solver_opts=dict(tol=1e-9), tol_gradient=1e-9)
    have = ~np.isnan(g['observed'])
    assert np.allclose(info[key]['synthetic'][have], g['synthetic'][have], rtol=1e-6)
    assert misfit == pytest.approx(float(g['misfit']), rel=1e-5)
    assert grad.shape == (2, nx, ny, nz)
    assert relerr(grad, g['gradient']) < 1e-5


def test_adjoint_gradient_vs_finite_differences():
    """The gradient is the derivative of the misfit: central differences of the misfit with
    respect to the resistivity of single cells (isotropic model, two sources, one frequency,
    both solves at tol 1e-10) agree with the adjoint-state gradient to 1 %, as in the
    reference's own test (tests/test_simulations.py: test_gradient / FD check)."""
    from emg3d_amd import gradient
    rng = np.random.default_rng(3)
    hx = widths(4, 3, 50., 1.3)
    hz = widths(4, 2, 40., 1.3)
    grid = emg3d.TensorMesh([hx, hx, hz], (-hx.sum() / 2, -hx.sum() / 2, -hz[:4].sum()))
    shape = grid.shape_cells
    rho = 10 ** rng.uniform(-0.2, 0.5, shape)
    srcs = {'a': (-60., 0., -30., 0., 0.), 'b': (40., 30., -30., 90., 0.)}
    freqs = {'f': 1.0}
    recs = np.array([[70., 10., -40., 0., 0.], [-30., -60., -40., 90., 0.], [10., 80., -25., 45., 0.]])
    true = emg3d.Model(grid, property_x=rho * (1 + 0.3 * rng.standard_normal(shape) * 0.5).clip(0.5, 2.0))
    opts = dict(tol=1e-10, sslsolver=True)
    obs = {}
    for s in srcs:
        ef = emg3d.solve(true, emg3d.get_source_field(grid, srcs[s], 1.0), **opts)
        obs[(s, 'f')] = emg3d.fields.get_receiver(ef, tuple(recs[:, k] for k in range(5)), 'linear')
    wts = {k: 1.0 / (0.05 * np.abs(v)) ** 2 for k, v in obs.items()}

    def phi(r):
        return gradient.misfit_and_gradient(emg3d.Model(grid, property_x=r), srcs, freqs, recs, obs, wts,
                                            solver_opts=opts, tol_gradient=1e-10)
    m0, g0, _ = phi(rho)
    assert g0.shape == shape and m0 > 0
    # as the reference's test does: cells with a sizeable gradient, away from boundary and sources
    cand = np.abs(g0).copy()
    cand[:2], cand[-2:], cand[:, :2], cand[:, -2:], cand[:, :, :2], cand[:, :, -2:] = 0, 0, 0, 0, 0, 0
    for s in srcs.values():
        i, j, k = (int(np.searchsorted(n, c)) - 1 for n, c in zip((grid.nodes_x, grid.nodes_y, grid.nodes_z), s[:3]))
        cand[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2, max(k - 1, 0):k + 2] = 0
    order = np.argsort(cand.ravel())[::-1][:3]
    for cell in (np.unravel_index(o, shape) for o in order):
        d = 1e-4 * rho[cell]
        rp = rho.copy()
        rp[cell] += d
        fd = (phi(rp)[0] - m0) / d
        nrmsd = 200 * abs(g0[cell] - fd) / (abs(g0[cell]) + abs(fd))
        assert nrmsd < 1.5, (cell, fd, g0[cell])


def test_residual_form_converges_to_roundoff_with_an_air_layer():
    """Multigrid as a solver on a marine model with an AIR layer of 1e8 Ohm m (the standard CSEM setting):
    the line smoothers multiply by stored block inverses, whose rounding errors (eps x cond of a block:
    1 / (omega mu sigma h^2) ~ 5e9 in the air) are relative to the right-hand side they are given. With
    the finest level in direct form that is the FIELD's scale and the residual stalls near 1e-8 of the
    source -- the reference reaches 1e-14 --; in residual form (`residual_form='auto'` switches it on
    for this model) it is the residual's scale: the iteration follows the oracle's (same ordering)
    history and converges to round-off like it. On a benign model both forms are the same iteration."""
    from bench import workload
    wl = workload('marine32')
    grid = emg3d.TensorMesh(wl['h'], wl['origin'])
    zc = np.broadcast_to(grid.cell_centers_z[None, None, :], grid.shape_cells)
    rh = np.where(zc > 0, 1e8, np.where(zc > -1000, 0.3, 1.0))
    rv = np.where(zc > 0, 1e8, np.where(zc > -1000, 0.3, 2.0))
    model = emg3d.Model(grid, property_x=rh, property_z=rv)
    sfield = emg3d.get_source_field(grid, wl['source'], 1.0)
    opts = dict(wl['opts'], sslsolver=False, tol=1e-12, maxit=40)
    e, info = emg3d.solve(model, sfield, return_info=True, **opts)                       # 'auto'
    assert info['exit'] == 0, info['exit_message']
    ed, infod = emg3d.solve(model, sfield, return_info=True, residual_form=False, **opts)
    assert infod['exit'] == 1 and infod['rel_error'] > 1e-10                             # the floor of the direct form
    og = mg_ref.Grid(grid.h, grid.origin)
    vm = mg_ref.volume_model(og, 1.0, 1 / rh, None, 1 / rv)
    oo = {k: v for k, v in opts.items() if k != 'sslsolver'}
    eo, io = mg_ref.solve(vm, mg_ref.Field(og, sfield.field.copy()), order=1, **oo)
    assert io['exit'] == 0 and abs(info['it_mg'] - io['it_mg']) <= 1
    n = min(len(info['error_at_cycle']), len(io['error_at_cycle'])) - 2
    assert np.allclose(info['error_at_cycle'][:n], io['error_at_cycle'][:n], rtol=2e-2)
    # (two fields with residuals of 1e-12 differ by 1e-7 here: the air makes the SYSTEM that ill-conditioned)
    assert relerr(e.field, eo.field) < 1e-6
    # benign model: the same iteration in both forms
    model2 = emg3d.Model(grid, property_x=np.where(zc > -1000, 0.3, 1.0), property_z=np.where(zc > -1000, 0.3, 2.0))
    o2 = dict(opts, tol=1e-9)
    _, ia = emg3d.solve(model2, sfield, return_info=True, residual_form=True, **o2)
    _, ib = emg3d.solve(model2, sfield, return_info=True, residual_form=False, **o2)
    assert ia['exit'] == ib['exit'] == 0 and ia['it_mg'] == ib['it_mg']
    assert np.allclose(ia['error_at_cycle'], ib['error_at_cycle'], rtol=1e-5)


@pytest.fixture(scope='module')
def stalled_case():
    """The solve of test_stalled_direct_form_continues_on_the_residual_equation (found by tools/soak_same_order.py:
    40^3, stretched 1.15, blocky tri-axial model, 0.5 Hz), the first tolerance under its direct form's floor with the
    direct-form solve that stalls there, and the single 'on-stall' solve at that tolerance."""
    import types
    rng = np.random.default_rng(83017)
    shape = (40, 40, 40)
    h = [widths(n // 2, n // 4, 25., 1.15) for n in shape]
    grid = emg3d.TensorMesh(h, [-w.sum() / 2 for w in h])
    shape = grid.shape_cells
    blocks = tuple(max(n // 8, 1) for n in shape)
    rho = np.kron(10 ** rng.uniform(-0.5, 1.5, blocks), np.ones([-(-n // b) for n, b in zip(shape, blocks)]))
    rho = np.asfortranarray(rho[:shape[0], :shape[1], :shape[2]])
    model = emg3d.Model(grid, rho, 1.5 * rho, 2.5 * rho)
    sfield = emg3d.get_source_field(grid, (10., -20., 30., 40., 10.), 0.5)
    kw = dict(sslsolver=False, cycle='F', semicoarsening=23, linerelaxation=7, nu_pre=1, nu_post=3, maxit=40)
    tol, infod = None, None
    for t in (1e-9, 3e-10, 1e-10, 3e-11):             # the first tolerance under the direct form's floor
        _, infod = emg3d.solve(model, sfield, tol=t, residual_form=False, return_info=True, **kw)
        if infod['exit'] == 1:
            tol = t
            break
    assert tol is not None and infod['exit_message'] == 'STAGNATED' and infod['residual_form'] is False
    e, info = emg3d.solve(model, sfield, tol=tol, residual_form='on-stall', return_info=True, **kw)
    # a second dipole on the same grid, for the batches
    sf2 = emg3d.get_source_field(grid, (-30., 10., -20., 10., 5.), 0.5)
    return types.SimpleNamespace(grid=grid, rho=rho, model=model, sfield=sfield, sf2=sf2, kw=kw, tol=tol, infod=infod,
                                 e=e, info=info)


def test_stalled_direct_form_continues_on_the_residual_equation(stalled_case):
    """A solve whose direct-form cycles stall above the tolerance (found by tools/soak_same_order.py: 40^3,
    stretched 1.15, blocky tri-axial model, 0.5 Hz, tol 1e-9 -- the direct form's floor is 1.7e-9 there, under
    the 'auto' rule's radar) must not return STAGNATED where the reference converges: with residual_form='auto'
    the cycling continues on the residual equation and converges; residual_form=False keeps the old behaviour;
    the oracle (same ordering) converges in 10 cycles."""
    c = stalled_case
    grid, rho, model, sfield, kw, tol, e, info = c.grid, c.rho, c.model, c.sfield, c.kw, c.tol, c.e, c.info
    assert info['exit'] == 0 and info['residual_form'] == 'switched', (info['exit_message'], info['residual_form'])
    # ('auto': since the rule knows about the conductivity contrast it starts this model in residual form --
    # and then needs the oracle's number of cycles)
    ea, infoa = emg3d.solve(model, sfield, tol=tol, return_info=True, **kw)
    assert infoa['exit'] == 0 and infoa['residual_form'] in (True, 'switched')
    og = mg_ref.Grid(grid.h, grid.origin)
    vm = mg_ref.volume_model(og, 0.5, 1 / rho, 1 / (1.5 * rho), 1 / (2.5 * rho))
    oo = {k: v for k, v in kw.items() if k != 'sslsolver'}
    eo, io = mg_ref.solve(vm, mg_ref.Field(og, sfield.field.copy()), tol=tol, order=1, **oo)
    assert io['exit'] == 0
    assert relerr(e.field, eo.field) < 1e-8
    assert io['it_mg'] < info['it_mg'] <= io['it_mg'] + 8         # the stall cost a few cycles, not the solve
    if infoa['residual_form'] is True:
        assert infoa['it_mg'] == io['it_mg'] and relerr(ea.field, eo.field) < 1e-9
    # a solve that converges in direct form is untouched
    _, i6 = emg3d.solve(model, sfield, tol=1e-6, return_info=True, **kw)
    assert i6['exit'] == 0 and i6['residual_form'] is False
    # in a batch the same happens for all its sources at once
    out = emg3d.solve_batch(model, [sfield, c.sf2], tol=tol, residual_form='on-stall', **kw)
    assert [i['exit'] for _, i in out] == [0, 0], [i['exit_message'] for _, i in out]
    assert relerr(out[0][0].field, eo.field) < 1e-8
    outd = emg3d.solve_batch(model, [sfield, c.sf2], tol=tol, residual_form=False, **kw)
    assert outd[0][1]['exit_message'] == 'STAGNATED'


def test_stalled_source_of_a_batch_switches_like_its_single_solve(stalled_case):
    """solve_batch(residual_form='on-stall') of the stalled source and a second dipole: the stalled source goes on
    on the residual equation as in its own solve -- it converges, reports 'switched', and its field is the single
    'on-stall' solve's to 1e-7 (until the switch the iterates are those of the single solve; after it the whole batch
    cycles on the residual equation, from the cycle at which the first of its sources stalled)."""
    c = stalled_case
    assert c.info['exit'] == 0 and c.info['residual_form'] == 'switched'
    out = emg3d.solve_batch(c.model, [c.sfield, c.sf2], tol=c.tol, residual_form='on-stall', **c.kw)
    eb, ib = out[0]
    d = relerr(eb.field, c.e.field)
    print(f"stalled source in a batch of two: exit {ib['exit']} ({ib['exit_message']}), residual_form "
          f"{ib['residual_form']!r}, {ib['it_mg']} cycles (single {c.info['it_mg']}), field vs single {d:.2e}")
    assert ib['exit'] == 0 and ib['residual_form'] == 'switched', (ib['exit_message'], ib['residual_form'])
    assert d < 1e-7, d


def test_volume_average_adjoint_is_the_transpose():
    """`_VolumeAverage.adjoint_add` (the gradient's way back from a computational grid, reference
    maps._interp_volume_average_adj) is the exact transpose of the linear averaging the same plan
    applies -- which is pinned to the reference's interp_volume_average
    (test_model_regridding_vs_reference_vectors): <P a, b> = <a, P^T b> for grids that are not
    nested, with the new grid both inside and beyond the original one; and P^T accumulates."""
    from emg3d_amd import models as emodels
    rng = np.random.default_rng(11)
    g1 = emg3d.TensorMesh([widths(5, 3, 30., 1.2), widths(4, 2, 40., 1.3), widths(6, 2, 25., 1.1)], (-200., -150., -300.))
    for h2, o2 in (([np.full(9, 47.), np.full(7, 61.), np.full(11, 33.)], (-150., -120., -250.)),      # inside
                   ([np.full(13, 53.), np.full(9, 71.), np.full(12, 49.)], (-330., -300., -380.))):   # beyond
        g2 = emg3d.TensorMesh(h2, o2)
        plan = emodels._VolumeAverage(g1, g2)
        a = rng.uniform(0.5, 2.0, g1.shape_cells)
        b = rng.standard_normal(g2.shape_cells)
        pa = plan(a, False)
        out = torch.full((g1.n_cells,), 0.25, dtype=torch.float64, device='cuda')
        plan.adjoint_add(torch.from_numpy(np.ascontiguousarray(b.ravel('F'))).cuda(), out)
        ptb = out.cpu().numpy().reshape(g1.shape_cells, order='F') - 0.25
        assert abs(np.vdot(pa, b) - np.vdot(a, ptb)) < 1e-12 * abs(np.vdot(pa, b))
        # a constant is reproduced, so P^T of the cell volumes returns the overlapped volume of every cell
        assert np.allclose(plan(np.ones(g1.shape_cells), False), 1.0, rtol=1e-13)


def test_adjoint_gradient_on_a_computational_grid_vs_finite_differences():
    """`misfit_and_gradient(grids=...)`: the pairs are solved on a computational grid that differs
    from the model grid (model there by volume averaging, cell gradient back through the adjoint of
    the averaging). With a conductivity model averaged linearly the chain is exact: central
    differences of the misfit -- computed through the same chain -- on the cells with the largest
    gradient agree to 1.5 %. (With the reference's default, averaging on a log10 scale, the way back
    is still the linear adjoint -- there as here -- and the agreement is ~10 %.) A computational grid
    equal to the model grid reproduces the plain result."""
    from emg3d_amd import gradient
    rng = np.random.default_rng(7)
    hx, hz = widths(4, 3, 50., 1.3), widths(4, 2, 40., 1.3)
    grid = emg3d.TensorMesh([hx, hx, hz], (-hx.sum() / 2, -hx.sum() / 2, -hz[:4].sum()))
    cx, cz = widths(6, 3, 35., 1.25), widths(6, 3, 28., 1.25)
    comp = emg3d.TensorMesh([cx, cx, cz], (-cx.sum() / 2, -cx.sum() / 2, -cz[:6].sum()))
    shape = grid.shape_cells
    rho = 10 ** rng.uniform(0.0, 0.3, shape)
    srcs = {'a': (-60., 0., -30., 0., 0.), 'b': (40., 30., -30., 90., 0.)}
    freqs = {'f': 1.0}
    recs = np.array([[70., 10., -40., 0., 0.], [-30., -60., -40., 90., 0.], [10., 80., -25., 45., 0.]])
    opts = dict(tol=1e-10, sslsolver=True)
    lin = {'log': False}
    true = emg3d.Model(grid, property_x=rho * 1.3, mapping='Conductivity').interpolate_to_grid(comp, **lin)
    obs = {}
    for s in srcs:
        ef = emg3d.solve(true, emg3d.get_source_field(comp, srcs[s], 1.0), **opts)
        obs[(s, 'f')] = emg3d.fields.get_receiver(ef, tuple(recs[:, k] for k in range(5)), 'linear')
    wts = {k: 1.0 / (0.05 * np.abs(v)) ** 2 for k, v in obs.items()}

    def phi(r, g):
        return gradient.misfit_and_gradient(emg3d.Model(grid, property_x=r, mapping='Conductivity'), srcs, freqs, recs,
                                            obs, wts, solver_opts=opts, tol_gradient=1e-10, grids=g, interpolate_opts=lin)
    m0, g0, _ = phi(rho, comp)
    assert g0.shape == shape and m0 > 0
    cand = np.abs(g0).copy()
    cand[:2], cand[-2:], cand[:, :2], cand[:, -2:], cand[:, :, :2], cand[:, :, -2:] = 0, 0, 0, 0, 0, 0
    order = np.argsort(cand.ravel())[::-1][:3]
    for cell in (np.unravel_index(o, shape) for o in order):
        d = 1e-4 * rho[cell]
        rp, rm = rho.copy(), rho.copy()
        rp[cell] += d
        rm[cell] -= d
        fd = (phi(rp, {('a', 'f'): comp, ('b', 'f'): comp})[0] - phi(rm, comp)[0]) / (2 * d)
        nrmsd = 200 * abs(g0[cell] - fd) / (abs(g0[cell]) + abs(fd))
        assert nrmsd < 1.5, (cell, fd, g0[cell])
    # a computational grid that IS the model grid (another object): the plain path
    same = emg3d.TensorMesh([hx, hx, hz], grid.origin)
    m1, g1, _ = phi(rho, same)
    m2, g2, _ = phi(rho, None)
    assert m1 == m2 and np.array_equal(g1, g2)


def test_magnetic_point_source_is_the_transpose_of_the_magnetic_receiver():
    """`fields.get_magnetic_point_source_field` (adjoint source of a magnetic point receiver, reference
    `_point_vector_magnetic`) is, entry by entry, the transpose of "H from E (`get_magnetic_field`, pinned to
    the reference's vectors), interpolated linearly to the point": <vector, e> equals the response for
    random fields, arbitrary orientations, points in stretched cells."""
    rng = np.random.default_rng(21)
    hx, hy, hz = widths(4, 3, 40., 1.3), widths(4, 2, 50., 1.25), widths(4, 3, 30., 1.4)
    grid = emg3d.TensorMesh([hx, hy, hz], (-hx.sum() / 2, -hy.sum() / 2, -hz.sum() / 2))
    model = emg3d.Model(grid, property_x=np.ones(grid.shape_cells))
    e = emg3d.Field(grid, frequency=0.8)
    e.field[:] = rng.standard_normal(e.field.size) + 1j * rng.standard_normal(e.field.size)
    h = emg3d.get_magnetic_field(model, e)
    recs = [(12.3, -7.1, 5.5, 0., 0.), (-40.2, 33.3, -20.1, 90., 0.), (3.3, 4.4, 18.8, 0., 90.),
            (-61.7, -48.2, 44.1, 37., -21.), (55.5, 12.1, -39.9, -120., 63.)]
    for rec in recs:
        resp = emg3d.fields.get_receiver(h, tuple(np.array([c]) for c in rec), 'linear')[0]
        src = emg3d.fields.get_magnetic_point_source_field(grid, rec, 0.8, strength=1.0)
        idx, val = src._sparse
        assert idx.size > 0 and np.array_equal(src.field[idx], val)
        got = np.sum(val / -src.smu0 * e.field[idx])
        assert abs(got - resp) < 1e-12 * abs(resp), (rec, got, resp)


def test_adjoint_gradient_with_magnetic_receivers_vs_finite_differences():
    """`misfit_and_gradient(magnetic=...)`: electric and magnetic point receivers in one data set;
    central differences of the misfit on the cells with the largest gradient agree to 1.5 %."""
    from emg3d_amd import gradient
    rng = np.random.default_rng(9)
    hx, hz = widths(4, 3, 50., 1.3), widths(4, 2, 40., 1.3)
    grid = emg3d.TensorMesh([hx, hx, hz], (-hx.sum() / 2, -hx.sum() / 2, -hz[:4].sum()))
    shape = grid.shape_cells
    rho = 10 ** rng.uniform(-0.2, 0.5, shape)
    srcs = {'a': (-60., 0., -30., 0., 0.), 'b': (40., 30., -30., 90., 0.)}
    freqs = {'f': 1.0}
    recs = np.array([[70., 10., -40., 0., 0.], [-30., -60., -40., 90., 0.], [10., 80., -25., 45., 0.],
                     [-75., 20., -35., 30., 20.]])
    mag = np.array([False, True, True, False])
    opts = dict(tol=1e-10, sslsolver=True)
    true = emg3d.Model(grid, property_x=rho * 1.4)
    obs = {}
    rt = tuple(recs[:, k] for k in range(5))
    for s in srcs:
        ef = emg3d.solve(true, emg3d.get_source_field(grid, srcs[s], 1.0), **opts)
        d = np.array(emg3d.fields.get_receiver(ef, rt, 'linear'))
        d[mag] = emg3d.fields.get_receiver(emg3d.get_magnetic_field(true, ef), tuple(r[mag] for r in rt), 'linear')
        obs[(s, 'f')] = d
    wts = {k: 1.0 / (0.05 * np.abs(v)) ** 2 for k, v in obs.items()}

    def phi(r):
        return gradient.misfit_and_gradient(emg3d.Model(grid, property_x=r), srcs, freqs, recs, obs, wts,
                                            solver_opts=opts, tol_gradient=1e-10, magnetic=mag)
    m0, g0, info = phi(rho)
    assert g0.shape == shape and m0 > 0

    def subset(sel, magnetic):
        return gradient.misfit_and_gradient(emg3d.Model(grid, property_x=rho), srcs, freqs, recs[sel],
                                            {k: v[sel] for k, v in obs.items()}, {k: v[sel] for k, v in wts.items()},
                                            solver_opts=opts, tol_gradient=1e-10, magnetic=magnetic)
    # misfit and gradient are sums over the data: electric subset + magnetic subset = the mixed set
    me, ge, _ = subset(~mag, None)
    mm, gm, _ = subset(mag, np.ones(mag.sum(), dtype=bool))
    assert mm > 0 and me > 0 and abs(me + mm - m0) < 1e-9 * m0
    assert relerr(ge + gm, g0) < 1e-6
    # finite differences on the MAGNETIC part (the electric one has its own test)
    phi = lambda r: gradient.misfit_and_gradient(                                   # noqa: E731
        emg3d.Model(grid, property_x=r), srcs, freqs, recs[mag], {k: v[mag] for k, v in obs.items()},
        {k: v[mag] for k, v in wts.items()}, solver_opts=opts, tol_gradient=1e-10, magnetic=np.ones(mag.sum(), dtype=bool))
    g0 = gm
    cand = np.abs(g0).copy()
    cand[:2], cand[-2:], cand[:, :2], cand[:, -2:], cand[:, :, :2], cand[:, :, -2:] = 0, 0, 0, 0, 0, 0
    for s in srcs.values():
        i, j, k = (int(np.searchsorted(n, c)) - 1 for n, c in zip((grid.nodes_x, grid.nodes_y, grid.nodes_z), s[:3]))
        cand[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2, max(k - 1, 0):k + 2] = 0
    order = np.argsort(cand.ravel())[::-1][:3]
    for cell in (np.unravel_index(o, shape) for o in order):
        d = 1e-4 * rho[cell]
        rp, rm = rho.copy(), rho.copy()
        rp[cell] += d
        rm[cell] -= d
        fd = (phi(rp)[0] - phi(rm)[0]) / (2 * d)
        nrmsd = 200 * abs(g0[cell] - fd) / (abs(g0[cell]) + abs(fd))
        assert nrmsd < 1.5, (cell, fd, g0[cell])


@pytest.mark.parametrize('freq', [1.3, -2.0])
def test_source_field_on_the_device_vs_host(freq):
    """the source vector of dipoles, finite dipoles and wires assembled by
    emg3d_dev_source_field (one thread per segment, walking from grid plane to grid plane) against
    the host get_source_field, which is pinned to the reference's fields (tests/test_host_api.py):
    point-like dipoles in all orientations, dipoles that end on nodes / run along grid lines and
    planes, a closed loop, a long wire through many cells; frequency and Laplace domain."""
    rng = np.random.default_rng(4)
    hx, hy, hz = widths(6, 3, 40., 1.3), widths(4, 3, 50., 1.25), widths(4, 2, 30., 1.4)
    grid = emg3d.TensorMesh([hx, hy, hz], (-hx.sum() / 2, -hy.sum() / 2, -hz[:5].sum()))
    nx_, ny_, nz_ = grid.nodes_x, grid.nodes_y, grid.nodes_z
    sources = [(0., 0., -20., 0., 0.), (13., -7., 5., 37., -21.), (-50., 20., -30., 90., 0.), (5., 5., 5., 0., 90.),
               (-20., 25., -3., -3., 7., 7.),                                     # finite, along x
               (nx_[3], nx_[7], ny_[2], ny_[2], nz_[4], nz_[4]),                 # on a grid line, node to node
               (nx_[2], nx_[9], ny_[1], ny_[6], nz_[2], nz_[5]),                 # node to node, diagonal
               (nx_[4], nx_[4], ny_[2] + 3., ny_[5] - 2., nz_[3], nz_[3]),       # inside a grid plane
               np.array([[-60., -40., -30.], [55., -35., -20.], [60., 45., 10.], [-50., 50., 0.], [-60., -40., -30.]]),
               np.cumsum(rng.uniform(-25., 40., (30, 3)), axis=0) * [1, 0.3, 0.1] + [-200., -60., -40.]]
    for src in sources:
        for strength in (1.0, 2.5 - 0.5j if freq > 0 else -1.5):
            host = emg3d.get_source_field(grid, src, freq, strength=strength)
            dev = emg3d.fields.source_field_device(grid, host._segments[0], freq, strength).cpu().numpy()
            assert relerr(dev, host.field) < 1e-13, (src, strength)
    # the path that uses it: parallel.solve's sparse upload goes through the device assembly
    model = emg3d.Model(grid, property_x=1.5)
    sf = emg3d.get_source_field(grid, sources[-2], freq)
    hier = solver.Hierarchy(emg3d.models.VolumeModel(model, sf))
    hier.put_source(sf, hier.top.s, sparse=True)
    assert relerr(hier.top.s.cpu().numpy(), sf.field) < 1e-13


@pytest.mark.gpu
def test_extrapolated_smoothing_same_solution_fewer_cycles():
    """solve(..., smoother_omega=1.3): every smoothing call is extrapolated (not in the reference;
    default 1 = the reference's smoothing). Same fixed point -- the converged field agrees with the
    plain solve to the tolerance -- and on the tri-axial workload, where the four-colour ordering
    costs cycles, it takes fewer; a batch gives the fields of the single solves."""
    import bench
    wl = bench.workload('triaxial64')
    grid = emg3d.TensorMesh(wl['h'], wl['origin'])
    model = emg3d.Model(grid, **{k: np.asfortranarray(v) for k, v in wl['res'].items()})
    sf = emg3d.get_source_field(grid, wl['source'], wl['frequency'])
    opts = dict(sslsolver=False, tol=1e-9, maxit=60, return_info=True, **wl['opts'])
    e1, i1 = emg3d.solve(model, sf, **opts)
    e2, i2 = emg3d.solve(model, sf, smoother_omega=1.3, **opts)
    assert i1['exit'] == 0 and i2['exit'] == 0
    assert i2['it_mg'] < i1['it_mg'], (i1['it_mg'], i2['it_mg'])
    assert np.linalg.norm(e1.field - e2.field) <= 2e-8 * np.linalg.norm(e1.field)
    sf2 = emg3d.get_source_field(grid, (150., -100., 50., 30., 10.), wl['frequency'])
    e3, i3 = emg3d.solve(model, sf2, smoother_omega=1.3, **opts)
    opts_b = {k: v for k, v in opts.items() if k != 'return_info'}
    (b2, ib2), (b3, ib3) = emg3d.solve_batch(model, [sf, sf2], smoother_omega=1.3, **opts_b)
    assert ib2['it_mg'] == i2['it_mg'] and ib3['it_mg'] == i3['it_mg']
    assert np.linalg.norm(b2.field - e2.field) <= 1e-12 * np.linalg.norm(e2.field)
    assert np.linalg.norm(b3.field - e3.field) <= 1e-12 * np.linalg.norm(e3.field)


# --- grid transfer, model restriction, residual and operator kernels through DeviceLevel, beyond one workgroup ----
# (shape, anisotropy case, with epsilon_r / mu_r). The launch block of these kernels is 64 x 4 threads, one plane
# (and, batched, one right-hand side) per blockIdx.z.
TRANSFER_SHAPES = [
    ((130, 6, 10), 'triaxial', False),    # 131 = 2 x 64 + 3 nodes in x (three threads in the last block); coarse: 66
    ((66, 70, 34), 'VTI', False),         # 67 nodes in x, 71 in y (18 rows of 4, three threads used); the coarse level
    #                                       (34 nodes in x) fits one block in x, the fine one does not; eta_y aliases eta_x
    ((10, 9, 130), 'HTI', True),          # odd in y (never coarsened), 131 planes: the batch index from blockIdx.z / planes
    ((64, 4, 2), 'isotropic', False),     # 65 = 64 + 1 nodes in x (one thread in the last block), a 2-cell direction in z
    ((2, 258, 6), 'triaxial', True),      # a 2-cell direction in x, 259 nodes in y (65 rows of 4, the last with 3)
    ((96, 129, 40), 'VTI', False),        # the largest (0.5 M cells): 97 nodes in x, 130 in y, odd in y
]
# odd everywhere: no coarsening; residual, operator and PEC kernels only. 64 and 128 nodes in x (last block full)
ODD_SHAPES = [((63, 5, 7), 'VTI', False), ((127, 11, 3), 'triaxial', True)]
TRANSFER_BATCHES = (1, 2, 5)
_SENTINEL = 7.5


def _ids(p):
    return 'x'.join(map(str, p[0])) + '-' + p[1] + ('-extras' if p[2] else '')


def _batch_calls(batch, nsrc=5):
    """Which of the nsrc test sources a level of `batch` right-hand sides is called with: alone, one call each,
    or the first `batch` together."""
    return [[b] for b in range(nsrc)] if batch == 1 else [list(range(batch))]


def _stack(fields, srcs):
    return torch.from_numpy(np.concatenate([fields[b].field for b in srcs]))


def test_transfer_shapes_cover_the_block_edges():
    """What TRANSFER_SHAPES / ODD_SHAPES promise: node counts of 64 k, 64 k + 1 and 64 k + 3 in x, y node counts that
    are and are not a multiple of 4, 2-cell directions, a coarse level inside one block of a fine one that is not, and
    every semicoarsening code admissible at least three times."""
    shapes = [s for s, _, _ in TRANSFER_SHAPES + ODD_SHAPES]
    xn = {(s[0] + 1) % 64 for s in shapes if s[0] + 1 >= 64}
    assert {0, 1, 3} <= xn
    assert any((s[1] + 1) % 4 for s in shapes) and any((s[1] + 1) % 4 == 0 for s in shapes)
    assert any(2 in s for s, _, _ in TRANSFER_SHAPES)
    assert any(s[0] + 1 > 64 >= s[0] // 2 + 1 for s, _, _ in TRANSFER_SHAPES)
    count = np.zeros(7, dtype=int)
    for s, _, _ in TRANSFER_SHAPES:
        count[admissible_sc_dirs(s)] += 1
    assert np.all(count >= 3), count
    assert all(admissible_sc_dirs(s) == [] for s in shapes[len(TRANSFER_SHAPES):])
    assert {c for _, c, _ in TRANSFER_SHAPES} == {'isotropic', 'VTI', 'HTI', 'triaxial'}


@pytest.mark.parametrize('dtype', [complex, float])
@pytest.mark.parametrize('shape,case,extras', TRANSFER_SHAPES, ids=map(_ids, TRANSFER_SHAPES))
def test_device_child_model_vs_oracle(shape, case, extras, dtype):
    """DeviceLevel.child(sc_dir) (k_restrict_param through emg3d_dev_restrict_param: grids of several blocks, ragged
    last blocks) against the coarse model of mg_ref.restriction, 1e-15, for every semicoarsening code the shape
    admits and levels of 1, 2 and 5 right-hand sides: summed eta_x / eta_y / eta_z / zeta, their aliasing as the
    anisotropy case says, the coarse widths, the sizes of the child's field buffers."""
    grid, vm, rng = random_level(shape, case, dtype, sum(shape), extras=extras, stretch=1.03)
    levels = [DeviceLevel.from_host(vm, torch.device('cuda'), batch=batch) for batch in TRANSFER_BATCHES]
    zero = mg_ref.Field(grid, dtype=dtype)
    for sc_dir, lv in [(sc_dir, lv) for sc_dir in admissible_sc_dirs(shape) for lv in levels]:
        cmodel = mg_ref.restriction(vm, zero, zero, sc_dir)[0]
        c = lv.child(sc_dir)['level']
        assert lv.child(sc_dir)['level'] is c
        assert c.grid.shape_cells == cmodel.grid.shape_cells == tuple(n // f for n, f in zip(shape, sc_factors(sc_dir)))
        for d in range(3):
            assert np.array_equal(c.grid.h[d], cmodel.grid.h[d]), (sc_dir, d)
            assert np.array_equal(c.ih[d].cpu().numpy(), 1.0 / cmodel.grid.h[d]), (sc_dir, d)
        for k in ('eta_x', 'eta_y', 'eta_z', 'zeta'):
            got = getattr(c, k).cpu().numpy()
            want = getattr(cmodel, k).ravel('F')
            assert got.dtype == want.dtype and got.shape == want.shape, (sc_dir, k)
            assert relerr(got, want) < 1e-15, (sc_dir, k)
        assert (c.eta_y is c.eta_x) == (cmodel.eta_y is cmodel.eta_x) == (case in ('isotropic', 'VTI')), sc_dir
        assert (c.eta_z is c.eta_x) == (cmodel.eta_z is cmodel.eta_x) == (case in ('isotropic', 'HTI')), sc_dir
        assert c.case == case and c.batch == lv.batch and c.flags == lv.flags
        assert c.e.numel() == c.s.numel() == lv.batch * c.grid.n_edges
    del levels, lv, c
    torch.cuda.empty_cache()


@pytest.mark.parametrize('dtype', [complex, float])
@pytest.mark.parametrize('shape,case,extras', TRANSFER_SHAPES, ids=map(_ids, TRANSFER_SHAPES))
def test_device_restrict_and_prolong_vs_oracle_single_and_batched(shape, case, extras, dtype):
    """DeviceLevel.restrict_to / prolong_from -- the path of a cycle: emg3d_dev_restrict_clear_batch and
    emg3d_dev_prolong_batch with the weights and tables of child() packed into one upload each, source b of a batch
    at b * n_edges -- for levels of 1, 2 and 5 right-hand sides and every admissible semicoarsening code, on five
    sources with different random data (non-zero on all boundary edges):

    * every source's coarse source equals mg_ref.restriction of ITS residual (1e-14), the coarse field, filled with a
      sentinel before, is exactly zero, and the batched call gives each source the bits of its own batch-1 call;
      emg3d_dev_restrict_batch (the entry without the clear) gives the same bits and leaves the coarse field alone;
    * every source's fine field after `+=` equals mg_ref.prolongation (1e-14), its PEC edges keep their bits, the
      coarse field is untouched, and batched equals single bit for bit."""
    grid, vm, rng = random_level(shape, case, dtype, sum(shape) + 1, extras=extras, stretch=1.03)
    dev = torch.device('cuda')
    n = grid.n_edges
    mask = pec_mask(grid)
    levels = {batch: DeviceLevel.from_host(vm, dev, batch=batch) for batch in TRANSFER_BATCHES}
    for sc_dir in admissible_sc_dirs(shape):
        cgrid = coarse_grid(grid, sc_dir)
        nc = cgrid.n_edges
        res = [random_field(grid, dtype, rng) for _ in range(5)]
        want_cs = [mg_ref.restriction(vm, r, r, sc_dir)[1].field for r in res]
        ces = [random_field(cgrid, dtype, rng) for _ in range(5)]
        fines = [random_field(grid, dtype, rng) for _ in range(5)]
        want_f = []
        for ce, f in zip(ces, fines):
            ref = f.copy()
            mg_ref.prolongation(ref, ce, sc_dir)
            want_f.append(ref.field)
        single_cs, single_f = {}, {}
        for batch, lv in levels.items():
            c = lv.child(sc_dir)['level']
            assert c.batch == batch and c.grid.n_edges == nc and c.s.numel() == batch * nc
            for srcs in _batch_calls(batch):
                at = (shape, sc_dir, batch, srcs)
                # restriction
                lv.r.copy_(_stack(res, srcs))
                c.s.fill_(_SENTINEL)
                c.e.fill_(_SENTINEL)
                assert lv.restrict_to(sc_dir) is c
                cs = c.s.cpu().numpy().reshape(batch, nc)
                assert not c.e.cpu().numpy().any(), at
                assert np.array_equal(lv.r.cpu().numpy(), _stack(res, srcs).numpy()), at
                for k, b in enumerate(srcs):
                    d = relerr(cs[k], want_cs[b])
                    assert d < 1e-14, (at, b, d)
                    if batch == 1:
                        single_cs[b] = cs[k].copy()
                    else:
                        assert np.array_equal(cs[k], single_cs[b]), (at, b)
                # the entry without the clear (emg3d_dev_restrict_batch), same weights: the bits of the coarse source
                # above, and a coarse field that keeps every bit of the sentinel
                c.s.fill_(_SENTINEL)
                c.e.fill_(_SENTINEL)
                _lib.check(_lib.lib().emg3d_dev_restrict_batch(
                    *c.parts(c.s), *lv.parts(lv.r), *lv.child(sc_dir)['wptr'], *shape, sc_dir, int(dtype is complex),
                    batch, n, nc, _stream()), 'emg3d_dev_restrict_batch')
                assert np.array_equal(c.s.cpu().numpy().reshape(batch, nc), cs), at
                kept = c.e.cpu().numpy()
                assert np.array_equal(kept.view(np.uint64), np.full_like(kept, _SENTINEL).view(np.uint64)), at
                assert np.array_equal(lv.r.cpu().numpy(), _stack(res, srcs).numpy()), at
                # prolongation
                c.e.copy_(_stack(ces, srcs))
                lv.e.copy_(_stack(fines, srcs))
                lv.prolong_from(sc_dir)
                got = lv.e.cpu().numpy().reshape(batch, n)
                assert np.array_equal(c.e.cpu().numpy(), _stack(ces, srcs).numpy()), at
                for k, b in enumerate(srcs):
                    d = relerr(got[k], want_f[b])
                    assert d < 1e-14, (at, b, d)
                    assert np.array_equal(got[k][mask], fines[b].field[mask]), (at, b)
                    assert np.any(got[k][~mask] != fines[b].field[~mask]) or mask.all(), (at, b)
                    if batch == 1:
                        single_f[b] = got[k].copy()
                    else:
                        assert np.array_equal(got[k], single_f[b]), (at, b)
    del levels, lv, c
    torch.cuda.empty_cache()


def _residual_checks(grid, vm, dtype, rng, levels, nsrc=5):
    """residual / residual_sumsq / apply_A of the levels {batch: DeviceLevel} of one model against core.amat_x of the
    oracle on nsrc sources with different random fields (non-zero on the boundary edges too); see
    test_device_residual_operator_and_pec_vs_oracle_single_and_batched."""
    n = grid.n_edges
    es = [random_field(grid, dtype, rng) for _ in range(nsrc)]
    ss = [random_field(grid, dtype, rng) for _ in range(nsrc)]
    want = []
    for e, s in zip(es, ss):
        r = s.copy()
        ocore.amat_x(r.fx, r.fy, r.fz, e.fx, e.fy, e.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h)
        want.append(r.field)
    single_r, single_norm = {}, {}
    for batch, lv in levels.items():
        for srcs in _batch_calls(batch, nsrc):
            at = (grid.shape_cells, batch, srcs)
            x, b_ = _stack(es, srcs).to(lv.device), _stack(ss, srcs).to(lv.device)
            lv.e.copy_(x)
            lv.s.copy_(b_)
            lv.r.fill_(_SENTINEL)
            norms = np.atleast_1d(lv.residual(store=True, norm=True))
            assert norms.shape == (batch,)
            got = lv.r.cpu().numpy().reshape(batch, n)
            for k, b in enumerate(srcs):
                d = relerr(got[k], want[b])
                assert d < 1e-13, (at, b, d)
                assert norms[k] == pytest.approx(np.linalg.norm(want[b]), rel=1e-12), (at, b)
                if batch == 1:
                    single_r[b], single_norm[b] = got[k].copy(), norms[k]
                else:
                    # "a source must get the same bits whether it is solved alone or in a batch" (launch_residual)
                    assert norms[k] == single_norm[b], (at, b, norms[k], single_norm[b])
                    assert np.array_equal(got[k], single_r[b]), (at, b)
            # store=False: the norm alone, r untouched
            lv.r.fill_(_SENTINEL)
            n2 = np.atleast_1d(lv.residual(store=False, norm=True))
            assert torch.all(lv.r == _SENTINEL).item(), at
            for k, b in enumerate(srcs):
                assert n2[k] == pytest.approx(np.linalg.norm(want[b]), rel=1e-12), (at, b)
            assert torch.equal(lv.e, x) and torch.equal(lv.s, b_), at
            # residual_sumsq on other tensors (_level_on): the norm of copying them into e, s; e, s, r untouched
            lv.e.fill_(_SENTINEL)
            lv.s.fill_(-_SENTINEL)
            sumsq = lv.residual_sumsq(x, b_)[:batch].cpu().numpy()
            assert np.array_equal(np.sqrt(sumsq), norms), (at, np.sqrt(sumsq), norms)
            assert torch.all(lv.e == _SENTINEL).item() and torch.all(lv.s == -_SENTINEL).item(), at
            assert torch.all(lv.r == _SENTINEL).item(), at
            # the Krylov operator on another tensor: A x = s - (s - A x)
            out = torch.full_like(x, float('nan'))
            assert lv.apply_A(x, out) is out
            o = out.cpu().numpy().reshape(batch, n)
            for k, b in enumerate(srcs):
                d = relerr(o[k], ss[b].field - want[b])
                assert d < 1e-12, (at, b, d)
            assert np.array_equal(x.cpu().numpy(), _stack(es, srcs).numpy()), at
            assert torch.all(lv.e == _SENTINEL).item() and torch.all(lv.r == _SENTINEL).item(), at


@pytest.mark.parametrize('dtype', [complex, float])
@pytest.mark.parametrize('shape,case,extras', TRANSFER_SHAPES + ODD_SHAPES, ids=map(_ids, TRANSFER_SHAPES + ODD_SHAPES))
def test_device_residual_operator_and_pec_vs_oracle_single_and_batched(shape, case, extras, dtype):
    """DeviceLevel.residual / residual_sumsq / apply_A / pec_zero (k_residual + k_reduce_sum, k_apply_operator,
    k_pec_zero) on levels of 1, 2 and 5 right-hand sides, five sources with different random fields and sources:

    * residual(store=True, norm=True): values against core.amat_x of the oracle per source (1e-13), one norm per
      source against the l2-norm of the oracle's residual (1e-12), batched values and norms bit-identical to the
      single-source ones (per-source partial sums [b nblk, (b+1) nblk), one k_reduce_sum workgroup per source);
    * store=False leaves r (a sentinel) alone;
    * residual_sumsq(x, b) on other tensors gives exactly the norm of copying them into e, s, and touches none of
      e, s, r;
    * apply_A(x, out) against s - residual of the oracle (1e-12);
    * pec_zero on ones: exactly the tangential boundary edges of every right-hand side become zero."""
    grid, vm, rng = random_level(shape, case, dtype, sum(shape) + 2, extras=extras, stretch=1.03)
    dev = torch.device('cuda')
    n = grid.n_edges
    levels = {batch: DeviceLevel.from_host(vm, dev, batch=batch) for batch in TRANSFER_BATCHES}
    _residual_checks(grid, vm, dtype, rng, levels)
    mask = pec_mask(grid)
    assert 0 < mask.sum() < n
    for batch, lv in levels.items():
        lv.e.fill_(1.0)
        lv.s.fill_(1.0)
        lv.pec_zero()
        got = lv.e.cpu().numpy().reshape(batch, n)
        for k in range(batch):
            assert np.array_equal(got[k] == 0, mask), (shape, batch, k)
            assert np.all(got[k][~mask] == 1), (shape, batch, k)
        assert torch.all(lv.s == 1.0).item()
    del levels, lv
    torch.cuda.empty_cache()


@pytest.mark.parametrize('dtype', [complex, float])
@pytest.mark.parametrize('roll', [1, 0])
def test_blocked_residual_with_ragged_last_blocks_vs_oracle(roll, dtype):
    """The residual and operator kernels with several planes per workgroup (option residual_zb; launch_residual and
    emg3d_dev_apply_operator take that path only where grid.x * grid.y * (planes / residual_zb) >= 8 x compute
    units -- asserted here from the device's CU count, so the case cannot fall back to one plane unnoticed) on a
    grid whose last x-block (131 = 2 x 64 + 3 nodes), last y-block (259 = 64 x 4 + 3) and last plane block (35 = 11
    x 3 + 2) are partly empty: with the column walk that carries operands between planes (residual_roll = 1,
    k_residual<T, true>) and cell by cell (0): values 1e-13, norms 1e-12 against the oracle, 1 and 2 right-hand
    sides, batched bit-identical to single."""
    shape, zb = (130, 258, 34), 3
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    gx, gy, planes = -(-(shape[0] + 1) // 64), -(-(shape[1] + 1) // 4), shape[2] + 1
    assert gx * gy * (planes // zb) >= 8 * cus, (gx, gy, planes, cus)
    assert (shape[0] + 1) % 64 and (shape[1] + 1) % 4 and planes % zb
    grid, vm, rng = random_level(shape, 'triaxial', dtype, 77 + roll, stretch=1.03)
    dev = torch.device('cuda')
    lib = _lib.lib()
    before = (lib.emg3d_get_option(b'residual_zb'), lib.emg3d_get_option(b'residual_roll'))
    try:
        assert lib.emg3d_set_option(b'residual_zb', zb) == 0 and lib.emg3d_set_option(b'residual_roll', roll) == 0
        assert (lib.emg3d_get_option(b'residual_zb'), lib.emg3d_get_option(b'residual_roll')) == (zb, roll)
        levels = {batch: DeviceLevel.from_host(vm, dev, batch=batch) for batch in (1, 2)}
        _residual_checks(grid, vm, dtype, rng, levels, nsrc=2)
    finally:
        lib.emg3d_set_option(b'residual_zb', before[0])
        lib.emg3d_set_option(b'residual_roll', before[1])
    assert (lib.emg3d_get_option(b'residual_zb'), lib.emg3d_get_option(b'residual_roll')) == before
    del levels
    torch.cuda.empty_cache()
