"""The NumPy model of the line smoothers with single-precision records (tests/compact_model.py) checked on the CPU --
the argument that tests/test_compact_records.py, which holds the HIP kernels against that model, means something:

V1  all roundings off, the model is the oracle's four-colour line smoother, and each of its line solves the dense
    numpy.linalg.solve of that line's system (assembly, block grouping, colour order -- nothing read from stencil.h);
V2  its index helper finds the records of the CPU walk's set-up (tests/emu), and the single-precision records of that
    set-up are the model's longdouble inverses correctly rounded;
V3  with the roundings of the streamed / the three-phase kernel switched on it is the CPU walk of that kernel, line by
    line, under the criterion of compact_model.Expectation;
V4  every rounding site alone is far above that criterion's threshold on more than 95 % of the lines: a kernel that
    rounds one value more or one value less than the model cannot pass.

Figures are printed and, with EMG3D_AMD_PARITY_FILE set, appended to that file (profiles/compact_records_parity.txt).
"""
import functools

import numpy as np
import pytest

import compact_model as cm
from emu import emu
from helpers import random_field
from oracle import core as ocore
from oracle import mg_ref
from test_sensitivity import record

SMOOTHERS = ('gauss_seidel', 'gauss_seidel_x', 'gauss_seidel_y', 'gauss_seidel_z')
STREAMED_CASES = [((130, 9, 30), 1), ((24, 20, 257), 3), ((20, 384, 22), 2), ((40, 40, 260), 3)]
THREE_PHASE_CASES = [((64, 40, 40), 1), ((40, 63, 40), 2), ((36, 36, 66), 3)]
FLIP_CAP = 0.05                      # share of the lines of a case that may lie above tau (never above d_line)


@functools.lru_cache(maxsize=None)
def level_and_model(shape, lr, dtype):
    grid, vm, s, e0 = cm.random_level(shape, lr, dtype)
    return grid, vm, s, e0, cm.LineModel(grid, vm, lr - 1, dtype)


@functools.lru_cache(maxsize=None)
def emu_expectation(shape, lr, dtype, streamed):
    """The model's expectation for a case on the single-precision records of the CPU walk's own set-up."""
    grid, vm, s, e0, model = level_and_model(shape, lr, dtype)
    fac, lfac = emu.line_setup(e0, s, vm, lr, compact=True)
    ex = cm.Expectation(model, e0.field, s.field, fac, cm.STREAMED if streamed else cm.THREE_PHASE)
    return ex, fac, lfac


def emu_smooth(e, s, vm, lr, nu, fac, lfac, mode, only=-1):
    out = e.copy()
    emu.lib().emu_set_line_compact(mode)
    emu.lib().emu_set_line_only(only)
    try:
        emu.gauss_seidel_fac(out, s, vm, lr, nu, fac, lfac)
    finally:
        emu.lib().emu_set_line_compact(0)
        emu.lib().emu_set_line_only(-1)
    return out


# ------------------------------------------------------------------------------------------------------------ V1
@pytest.mark.parametrize('shape,lr', [((12, 9, 10), 1), ((9, 13, 8), 2), ((8, 9, 17), 3), ((37, 6, 7), 1)])
@pytest.mark.parametrize('dtype', [complex, float])
def test_v1_model_without_roundings_is_the_oracle_and_a_dense_solve(shape, lr, dtype):
    grid, vm, s, e0 = cm.random_level(shape, lr, dtype)
    model = cm.LineModel(grid, vm, lr - 1, dtype)
    # the assembled matrix against one product of the oracle's operator
    x, r = random_field(grid, dtype, np.random.default_rng(1)), mg_ref.Field(grid, dtype=dtype)
    ocore.amat_x(r.fx, r.fy, r.fz, x.fx, x.fy, x.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h)
    assert np.abs(-r.field - model.A @ x.field).max() < 1e-14 * np.abs(r.field).max()
    args = (s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h)
    for nu in (1, 3):
        a = e0.copy()
        getattr(ocore, SMOOTHERS[lr])(a.fx, a.fy, a.fz, *args, nu, order=1)
        xl = model.smooth(e0.field, s.field, nu)
        xd = model.smooth(e0.field, s.field, nu, longdouble=False)
        spread = cm.line_distance(model, xd, xl).max()
        d = cm.line_distance(model, a.field, xl).max()
        record(f"V1 {shape} lr={lr} {dtype.__name__} nu={nu}: model vs oracle {d:.2e}, float64-vs-longdouble spread {spread:.2e}")
        assert d <= 10 * spread
    # every line solve of one pass against numpy's dense solve of that line's system
    A = model.A.tocsr()
    for colour in (1, 2):
        e = e0.field.astype(np.clongdouble if dtype is complex else np.longdouble)
        e64 = e0.field.copy()
        model.colour_pass(colour, e, s.field.astype(e.dtype), e.dtype)
        model.colour_pass(colour, e64, s.field, e64.dtype)
        res = s.field - A @ e0.field
        for pos, xm, x64 in zip(model.line_unknowns(colour), e[model.line_unknowns(colour)], e64[model.line_unknowns(colour)]):
            Al = A[pos][:, pos].toarray()
            xs = np.linalg.solve(Al, res[pos] + Al @ e0.field[pos])
            scale = np.abs(xm).max()
            assert np.abs(xs - xm).max() / scale <= 10 * max(np.abs(x64 - xm).max() / scale, 1e-15 * np.linalg.cond(Al))


# ------------------------------------------------------------------------------------------------------------ V2
@pytest.mark.parametrize('shape,lr', [((130, 9, 30), 1), ((11, 36, 10), 2), ((9, 12, 41), 3)])
@pytest.mark.parametrize('dtype', [complex, float])
def test_v2_record_layout_and_single_precision_records_of_the_cpu_setup(shape, lr, dtype):
    grid, vm, s, e0 = cm.random_level(shape, lr, dtype)
    model = cm.LineModel(grid, vm, lr - 1, dtype)
    wt = np.clongdouble if dtype is complex else np.longdouble
    fac64, _ = emu.line_setup(e0, s, vm, lr)
    worst = 0.0
    for c in range(4):          # the index helper: every fp64 record is the model's inverse of that line and block
        T, TQ = model.own_records(c, wt)
        D, DQ = model.own_records(c, fac64.dtype)
        S, SQ = model.buffer_records(c, fac64)
        for t, d, st in [(T[k], D[k], S[k]) for k in T] + [(TQ, DQ, SQ)]:
            err = np.abs(st - t).max(axis=(1, 2)) / np.abs(t).max(axis=(1, 2))
            spread = np.abs(d - t).max(axis=(1, 2)) / np.abs(t).max(axis=(1, 2))
            assert err.max() <= 10 * spread.max()           # (a record of another line or block is off by O(1))
            worst = max(worst, float(err.max() / spread.max()))
    fac32, _ = emu.line_setup(e0, s, vm, lr, compact=True)
    assert fac32.dtype == (np.complex64 if dtype is complex else np.float32) and fac32.size == fac64.size
    ulps, rel = cm.record_errors(model, fac32)
    record(f"V2 {shape} lr={lr} {dtype.__name__}: fp64 records vs longdouble inverses, worst error / float64-vs-longdouble "
           f"spread of the block {worst:.1f}; single-precision records: worst error {ulps:.3f} fp32 ulps (record distance {rel:.1e})")
    assert ulps <= 0.5
    assert 1e-9 < rel < 1e-6


# ------------------------------------------------------------------------------------------------------------ V3
def _v3(shape, lr, dtype, streamed):
    grid, vm, s, e0, model = level_and_model(shape, lr, dtype)
    ex, fac, lfac = emu_expectation(shape, lr, dtype, streamed)
    mode, name = (1, 'streamed') if streamed else (2, 'three-phase')
    cap = FLIP_CAP if streamed else 0            # (w kept in fp64: nothing can flip)
    assert ex.tau_is_tight(), (ex.tau, np.median(ex.d_line))
    # pass by pass through the first sweep, model and CPU walk from the same state: every line once
    state, tot = e0.copy(), np.zeros(3, int)
    worst = 0.0
    for c in cm.sweep_colours(1):
        state = emu_smooth(state, s, vm, lr, 1, fac, lfac, mode, only=c)
        above, beyond, lines, ratio = ex.compare_pass(state.field, c)
        tot, worst = tot + (above, beyond, lines), max(worst, ratio)
    line = (f"V3 {name} {shape} lr={lr} {dtype.__name__}: tau {ex.tau:.2e} (median d_line {np.median(ex.d_line):.2e}); "
            f"pass by pass {tot[0]}/{tot[2]} lines above tau, worst delta/d {worst:.1e}")
    assert tot[0] <= cap * tot[2] and tot[1] == 0, line
    # the lines of the last pass of whole calls: nu = 1 .. 4 end with the classes 0, 3, 2, 1
    for nu in ((1, 2, 3, 4) if np.prod(shape) < 130000 else (1, 3)):       # (the first sweep above holds every class)
        out = emu_smooth(e0, s, vm, lr, nu, fac, lfac, mode)
        above, beyond, lines, ratio = ex.compare_last_pass(out.field, nu)
        line += f"; nu={nu} last pass {above}/{lines}, {ratio:.1e}"
        assert above <= cap * lines and beyond == 0, line
        # the whole call from the start field: the criterion itself without flips, figures with them (on the smaller levels)
        if nu in (1, 3) and (not streamed or np.prod(shape) < 130000):
            share, ratio, l2 = ex.compare(out.field, nu)
            line += f", whole call {100 * share:.1f} % above tau, worst delta/d {ratio:.1e}, rel-L2 {l2:.1e}"
            assert streamed or share == 0, line
    record(line)


@pytest.mark.parametrize('shape,lr', STREAMED_CASES)
@pytest.mark.parametrize('dtype', [complex, float])
def test_v3_model_with_T_w_and_middle_rhs_rounded_is_the_streamed_cpu_walk(shape, lr, dtype):
    _v3(shape, lr, dtype, True)


@pytest.mark.parametrize('shape,lr', THREE_PHASE_CASES)
@pytest.mark.parametrize('dtype', [complex, float])
def test_v3_model_with_T_rounded_is_the_three_phase_cpu_walk(shape, lr, dtype):
    _v3(shape, lr, dtype, False)


# ------------------------------------------------------------------------------------------------------------ V4
@pytest.mark.parametrize('shape,lr,streamed', [((130, 9, 30), 1, True), ((24, 20, 257), 3, True), ((64, 40, 40), 1, False),
                                               ((36, 36, 66), 3, False)])
@pytest.mark.parametrize('dtype', [complex, float])
def test_v4_each_rounding_site_alone_is_detectable(shape, lr, streamed, dtype):
    """One pass of every colour class from the same state with the model's own records: the kernel's set of roundings
    against that set with one switch turned the other way. tau: that of the case (V3)."""
    grid, vm, s, e0, model = level_and_model(shape, lr, dtype)
    tau = emu_expectation(shape, lr, dtype, streamed)[0].tau
    base = dict(cm.STREAMED if streamed else cm.THREE_PHASE)
    wt = np.clongdouble if dtype is complex else np.longdouble
    sl = s.field.astype(wt)
    moved = {k: [] for k in base}
    moved_q = []
    for c in range(4):
        ref = e0.field.astype(wt)
        model.colour_pass(c, ref, sl, wt, **base)
        for k in base:
            x, tr = e0.field.astype(wt), {}
            model.colour_pass(c, x, sl, wt, trace=tr, **{**base, k: not base[k]})
            moved[k].append(cm.pass_distance(model, c, x, ref) > tau)
            if k == 'round_middle_rhs':
                q = model.mid(c)
                moved_q.append(np.abs(x[q] - ref[q]).max(1) / np.abs(ref[q]).max(1) > tau)
    shares = {k: float(np.concatenate(v).mean()) for k, v in moved.items()}
    shares['round_middle_rhs (Q only)'] = float(np.concatenate(moved_q).mean())
    record(f"V4 {'streamed' if streamed else 'three-phase'} {shape} lr={lr} {dtype.__name__}: share of the lines a single "
           f"switch moves past tau = {tau:.1e}: " + ', '.join(f"{k} {100 * v:.1f} %" for k, v in shares.items()))
    assert all(v > 0.95 for v in shares.values()), shares


# ------------------------------------------------------------------------- the eta sums of the tiled point smoother
POINT_SHAPES = [(36, 20, 18), (40, 24, 33)]
POINT_VARIANTS = [(complex, False), (float, False), (complex, True)]
POINT_TOL = 5e-10            # the per-sweep bound of the tiled point smoother against the oracle's tile order


def point_level(shape, dtype, extras):
    return cm.random_level(shape, 0, dtype, seed=sum(shape) + 3, freq=3e6 if extras else 1.3, extras=extras)


def point_tolerance(on, off):
    """The bound of a comparison with the oracle's rounded sums: the kernel's per-sweep bound, and no more than a
    two-hundredth of what the rounding changes in the oracle itself (six sums per node in single precision move a sweep
    by 1e-8 ... 3e-8, less than 100 x 5e-10) -- so that the oracle with fp64 sums is always more than 100 bounds away
    from a result within the bound, and the comparison tells the two apart."""
    from helpers import relerr
    return min(POINT_TOL, relerr(on, off) / 200)


def oracle_point_sweeps(grid, vm, s, e0, nu, rounded):
    """nu sweeps of the oracle's point smoother in tile order, its eta sums rounded to single precision or not."""
    a = e0.copy()
    ocore.set_eta_sum_round(rounded)
    try:
        ocore.gauss_seidel(a.fx, a.fy, a.fz, s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h, nu, order=2)
    finally:
        ocore.set_eta_sum_round(False)
    return a.field


@pytest.mark.parametrize('shape', POINT_SHAPES)
@pytest.mark.parametrize('dtype,extras', POINT_VARIANTS)
def test_oracle_eta_sum_rounding_is_the_cpu_walk_of_the_compact_point_smoother(shape, dtype, extras):
    """oracle_set_eta_sum_round against the CPU walk of the tiled point smoother with single-precision sums (stored
    halves for nu = 1, full values for nu = 3): within the bound of `point_tolerance`, and the oracle with fp64 sums
    more than 100 bounds away -- the comparison sees the rounding."""
    from helpers import relerr
    grid, vm, s, e0 = point_level(shape, dtype, extras)
    for nu in (1, 3):
        ref = e0.copy()
        emu.lib().emu_set_point_tile_min(1)
        emu.lib().emu_set_point_compact(1)
        try:
            emu.gauss_seidel(ref, s, vm, 0, nu)
        finally:
            emu.lib().emu_set_point_compact(0)
            emu.lib().emu_set_point_tile_min(1 << 20)
        on, off = (oracle_point_sweeps(grid, vm, s, e0, nu, r) for r in (True, False))
        record(f"eta sums {shape} {dtype.__name__}{' extras' if extras else ''} nu={nu}: CPU walk vs oracle with rounded sums "
               f"{relerr(ref.field, on):.1e}, with fp64 sums {relerr(ref.field, off):.1e}")
        tol = point_tolerance(on, off)
        assert relerr(ref.field, on) < tol
        assert relerr(ref.field, off) > 100 * tol
