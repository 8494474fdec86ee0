"""GPU side of the parity of the single-precision ("compact") smoother records -- the product default on correction
levels -- against checkers that do not share the kernels' code:

* k_line_stream<.., COMPACT> (T and w records and the middle block's right-hand side in fp32) and k_line_colour with
  compact T records against tests/compact_model.py, a NumPy model in longdouble whose operator comes from the oracle's
  amat_x; tests/test_compact_model.py carries the argument that the model is right and that every rounding site alone is
  visible. The model runs on the T records the HIP set-up stored, which are checked themselves: every entry the
  model's own longdouble inverse, correctly rounded.
  The per-line criterion (compact_model.Expectation): delta_line <= tau (1e-12 ... 1e-10, more than a thousand times
  below what one rounding site is worth); the lines where an fp64 evaluation of a w entry falls on the other side of an
  fp32 rounding boundary than the model's may exceed tau, never d_line, and are at most 5 % of the lines compared. It is
  applied to the lines of the LAST pass of calls of nu = 1, 2, 3, 4 sweeps (they end with the colour classes 0, 3, 2,
  1: every line of the level once), the model's pass taken from the kernel's own final field: a flipped line's
  neighbours read its values in the next pass, so followed from the start field one flip reaches every line within
  nine passes (on the CPU walk, whole calls of nu = 3: 19 % / 37 % of the lines of (24, 20, 257) above tau from 2 / 6
  flips per sweep -- profiles/compact_records_parity.txt). Without w rounding (three-phase kernel) nothing flips and
  the whole call from the start field is held to tau as well, on every line.
* the tiled point smoother's single-precision eta sums against the oracle with oracle_set_eta_sum_round;
* a Krylov solve whose finest level streams compact records against the oracle's converged field.

Figures are printed and, with EMG3D_AMD_PARITY_FILE set, appended to that file (profiles/compact_records_parity.txt).
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import compact_model as cm
import emg3d_amd as emg3d
from emg3d_amd import _lib, solver
from emg3d_amd._device import DeviceLevel
from helpers import relerr, widths
from oracle import mg_ref
from test_compact_model import (FLIP_CAP, POINT_SHAPES, POINT_VARIANTS, STREAMED_CASES, THREE_PHASE_CASES, level_and_model,
                                oracle_point_sweeps, point_level, point_tolerance)
from test_gpu_parity import _option
from test_sensitivity import record

pytestmark = pytest.mark.gpu
NUS = (1, 2, 3, 4)


@functools.lru_cache(maxsize=None)
def gpu_case(shape, lr, dtype, streamed):
    """One level on the GPU with compact records: the fields after nu = 1 .. 4 sweeps, the stored T records, and the
    model's expectation on those records (built once per case)."""
    lib = _lib.lib()
    grid, vm, s, e0, model = level_and_model(shape, lr, dtype)
    want = b'k_line_stream' if streamed else b'k_line_colour'
    out = {}
    # (real 130-block lines: the fp64 records of 16 lines fit the LDS of a CU and the level would run k_line_colour --
    #  without LDS records it streams like the others)
    with contextlib.ExitStack() as stack:
        stack.enter_context(_option('line_lpw', 16 if streamed else 0))
        if streamed and lib.emg3d_line_kernel_name(lr, *shape, int(dtype is complex), 1) != want:
            stack.enter_context(_option('line_lds', 0))
        assert lib.emg3d_line_kernel_name(lr, *shape, int(dtype is complex), 1) == want
        lv = DeviceLevel.from_host(vm, torch.device('cuda'))
        lv.set_line_compact(True)
        assert lib.emg3d_line_compact_used(lv._cref, lr) == 1
        lv.s.copy_(torch.from_numpy(s.field))
        for nu in NUS:
            lv.e.copy_(torch.from_numpy(e0.field))
            lv.smooth(lr, nu)
            out[nu] = lv.e.cpu().numpy()
        fac = lv.line_factors(lr)[0].cpu().numpy().view(np.complex64 if dtype is complex else np.float32)
        assert fac.size == 15 * cm.line_padded(shape[lr - 1]) * int(cm.line_offsets(model)[-1])      # nothing but T records, in single precision
    ex = cm.Expectation(model, e0.field, s.field, fac, cm.STREAMED if streamed else cm.THREE_PHASE)
    return out, fac, ex


def _name(shape, lr, dtype, streamed):
    return f"{'k_line_stream' if streamed else 'k_line_colour'} {shape} lr={lr} {dtype.__name__}"


def _records(shape, lr, dtype, streamed):
    out, fac, ex = gpu_case(shape, lr, dtype, streamed)
    ulps, rel = cm.record_errors(ex.model, fac)
    record(f"{_name(shape, lr, dtype, streamed)}: stored T records vs the model's longdouble inverses: worst error "
           f"{ulps:.3f} fp32 ulps, record distance {rel:.1e}; tau {ex.tau:.2e}, median d_line {np.median(ex.d_line):.2e}")
    assert ulps <= 0.5
    assert 1e-9 < rel < 1e-6            # really single precision
    assert ex.tau_is_tight(), (ex.tau, np.median(ex.d_line))


def _lines(shape, lr, dtype, streamed, nu):
    out, fac, ex = gpu_case(shape, lr, dtype, streamed)
    e0 = level_and_model(shape, lr, dtype)[3]
    assert np.any(out[nu] != e0.field)
    above, beyond, lines, ratio = ex.compare_last_pass(out[nu], nu)
    line = (f"{_name(shape, lr, dtype, streamed)} nu={nu}: last pass {above}/{lines} lines above tau = {ex.tau:.1e} "
            f"({100 * above / lines:.2f} %), worst delta/d {ratio:.1e}")
    if not streamed and nu in (1, 3):
        share, wratio, l2 = ex.compare(out[nu], nu)
        line += f"; whole call {100 * share:.2f} % above tau, worst delta/d {wratio:.1e}, rel-L2 {l2:.1e}"
        assert share == 0, line
    record(line)
    assert above <= (FLIP_CAP * lines if streamed else 0) and beyond == 0, line


@pytest.mark.parametrize('shape,lr', STREAMED_CASES)
@pytest.mark.parametrize('dtype', [complex, float])
def test_streamed_kernel_setup_stores_correctly_rounded_records(shape, lr, dtype):
    _records(shape, lr, dtype, True)


@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('shape,lr', STREAMED_CASES)
@pytest.mark.parametrize('dtype', [complex, float])
def test_streamed_kernel_lines_vs_model(shape, lr, dtype, nu):
    _lines(shape, lr, dtype, True, nu)


@pytest.mark.parametrize('shape,lr', THREE_PHASE_CASES)
@pytest.mark.parametrize('dtype', [complex, float])
def test_three_phase_kernel_setup_stores_correctly_rounded_records(shape, lr, dtype):
    _records(shape, lr, dtype, False)


@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('shape,lr', THREE_PHASE_CASES)
@pytest.mark.parametrize('dtype', [complex, float])
def test_three_phase_kernel_lines_vs_model(shape, lr, dtype, nu):
    _lines(shape, lr, dtype, False, nu)


@pytest.mark.parametrize('dtype', [complex, float])
def test_streamed_compact_batch_of_three_equals_single_sources(dtype):
    """The project's rule on the compact path: each right-hand side of a batch bit for bit its single-source result."""
    shape, lr = STREAMED_CASES[1]
    lib = _lib.lib()
    grid, vm, s, e0, _ = level_and_model(shape, lr, dtype)
    rng = np.random.default_rng(3)
    n = e0.field.size
    srcs = [s.field * (1 + b) + (0.3 * b) * rng.standard_normal(n) for b in range(3)]
    starts = [e0.field * (1.0 - 0.2 * b) for b in range(3)]
    dev = torch.device('cuda')
    with _option('line_lpw', 16):
        single = DeviceLevel.from_host(vm, dev)
        single.set_line_compact(True)
        many = DeviceLevel.from_host(vm, dev, batch=3)
        many.set_line_compact(True)
        assert lib.emg3d_line_compact_used(single._cref, lr) == 1 and lib.emg3d_line_compact_used(many._cref, lr) == 1
        want = []
        for b in range(3):
            single.s.copy_(torch.from_numpy(srcs[b]))
            single.e.copy_(torch.from_numpy(starts[b]))
            single.smooth(lr, 3)
            want.append(single.e.cpu().numpy())
        many.s.copy_(torch.from_numpy(np.concatenate(srcs)))
        many.e.copy_(torch.from_numpy(np.concatenate(starts)))
        many.smooth(lr, 3)
        got = many.e.cpu().numpy().reshape(3, n)
    assert np.array_equal(want[0], gpu_case(shape, lr, dtype, True)[0][3])          # (source 0 is the case's own)
    for b in range(3):
        assert np.any(want[b] != starts[b])
        assert np.array_equal(got[b], want[b]), (b, relerr(got[b], want[b]))


@pytest.mark.parametrize('shape', POINT_SHAPES)
@pytest.mark.parametrize('dtype,extras', POINT_VARIANTS)
def test_point_tiled_compact_eta_sums_vs_oracle(shape, dtype, extras):
    """The tiled point smoother with its six eta edge sums per node in single precision (POINT_COMPACT) against the
    oracle in tile order with the same rounding (oracle_set_eta_sum_round), at the kernel's per-sweep bound (tightened
    where needed so that the oracle with fp64 sums is more than 100 bounds away: test_compact_model.point_tolerance)."""
    lib = _lib.lib()
    grid, vm, s, e0 = point_level(shape, dtype, extras)
    with _option('point_tile_min', 1):
        lv = DeviceLevel.from_host(vm, torch.device('cuda'))
        lv.set_line_compact(True)
        assert lib.emg3d_point_compact_used(lv._cref)
        lv.s.copy_(torch.from_numpy(s.field))
        for nu in (1, 2):
            lv.e.copy_(torch.from_numpy(e0.field))
            lv.smooth(0, nu)
            got = lv.e.cpu().numpy()
            on, off = (oracle_point_sweeps(grid, vm, s, e0, nu, r) for r in (True, False))
            tol = point_tolerance(on, off)
            record(f"k_gs_point_tile compact sums {shape} {dtype.__name__}{' extras' if extras else ''} nu={nu}: vs oracle with "
                   f"rounded sums {relerr(got, on):.1e} (bound {tol:.1e}), with fp64 sums {relerr(got, off):.1e}")
            assert relerr(got, on) < tol
            assert relerr(got, off) > 100 * tol


def test_krylov_with_compact_records_on_a_level_that_streams():
    """BiCGSTAB preconditioned by multigrid with x-line relaxation on 192 x 16 x 16 cells: 192-block lines stream their
    records in every mode. fp64 records and the default ('auto': compact here) end alike, need the same iterations
    (+- 1) and give the oracle's converged field."""
    lib = _lib.lib()
    shape = (192, 16, 16)
    h = [widths(160, 16, 50., 1.1), widths(8, 4, 50., 1.2), widths(8, 4, 50., 1.2)]
    grid = emg3d.TensorMesh(h, [-w.sum() / 2 for w in h])
    assert grid.shape_cells == shape
    rng = np.random.default_rng(192)
    rho = 10 ** rng.uniform(-0.5, 0.5, shape)
    model = emg3d.Model(grid, rho, 1.5 * rho, 2.0 * rho)
    freq = 1.0
    sfield = emg3d.get_source_field(grid, (20., 5., -10., 30., 10.), freq)
    vmodel = emg3d.models.VolumeModel(model, sfield)
    assert solver.block_condition(vmodel) <= solver.COMPACT_COND_MAX
    ogrid = mg_ref.Grid(grid.h, grid.origin)
    vm = mg_ref.volume_model(ogrid, freq, 1 / rho, 1 / (1.5 * rho), 1 / (2.0 * rho))
    eo, io = mg_ref.solve(vm, mg_ref.Field(ogrid, sfield.field.copy()), tol=1e-10, linerelaxation=1)
    assert io['exit'] == 0
    res = {}
    with _option('line_lpw', 16):
        assert lib.emg3d_line_kernel_name(1, *shape, 1, 1) == b'k_line_stream'
        for compact in (False, 'auto'):
            hier = solver.Hierarchy(vmodel, line_compact=compact, point_compact_top=True)
            e, info = emg3d.solve(model, sfield, sslsolver=True, tol=1e-8, linerelaxation=1, return_info=True,
                                  hierarchy=hier, line_compact=compact)
            assert bool(info['line_compact']) == bool(compact) and hier.top.uses_line_compact() == bool(compact)
            assert bool(lib.emg3d_line_compact_used(hier.top._cref, 1)) == bool(compact)
            res[compact] = (e.field.copy(), info)
            record(f"Krylov {shape} line_compact={compact!r}: exit {info['exit']}, {info['it_ssl']} iterations, "
                   f"{info['it_mg']} cycles, vs the oracle's converged field {relerr(e.field, eo.field):.1e}")
    (ea, ia), (eb, ib) = res[False], res['auto']
    assert ia['exit'] == ib['exit'] == 0
    assert abs(ia['it_ssl'] - ib['it_ssl']) <= 1
    assert relerr(ea, eo.field) < 1e-8 and relerr(eb, eo.field) < 1e-8
