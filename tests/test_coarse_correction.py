"""What sits underneath every coarse-grid correction (-m gpu):

A. ``k_gs_point_small``, the one-workgroup point smoother of the coarsest levels (option point_small: every colour pass
   of a call in one launch, two bits per pass in one 64-bit word), against the launch-per-colour path bit for bit and
   against the oracle in the same order -- at the 512-node threshold, with a second round of its stride loop, with one
   and two interior nodes, and with 16, 20, 29, 32 and (fallback) 36 passes per call;
B. a coarse-grid correction replayed from a captured HIP graph against the same correction launched eagerly, bit for
   bit, for every kind of solve that reaches the replay; and a second solve on the same hierarchy, whose replays start
   behind another cycle than they were captured behind (where one chain of coarse levels meets every line-relaxation
   code, that needs Workspace.factor_epoch);
C. a ``Hierarchy`` that is reused after ``emg3d_set_option`` against a fresh one under the same options, bit for bit,
   and what ``_cycle._purge_stale_graphs`` / ``_drop_stale_factors`` promise about its caches.

Figures printed here (run with -s) are the source of profiles/coarse_correction_tests.txt.
"""
import numpy as np
import pytest
import torch

import emg3d_amd as emg3d
from emg3d_amd import _cycle, _lib, core, solver
from emg3d_amd._device import DeviceLevel, _stream
from oracle import core as ocore
from helpers import random_field, random_level, relerr, widths

pytestmark = pytest.mark.gpu

# option defaults (include/emg3d_amd.h) of everything these tests touch: what every `finally` goes back to
DEFAULTS = {'point_small': 512, 'skip_repeat': 1, 'point_order': 1, 'line_fuse': 2, 'line_lds': 1, 'line_lpw': 0,
            'residual_zb': 8, 'line_order': 1, 'line_wide': 33, 'point_tile_min': 1 << 20, 'point_compact': 0,
            'line_compact': 0}


def _set(name, value):
    assert _lib.lib().emg3d_set_option(name.encode(), int(value)) == 0, (name, value)


def _restore_defaults():
    for name, value in DEFAULTS.items():
        _lib.lib().emg3d_set_option(name.encode(), value)
    ocore.lib().oracle_set_point_repeat(1)


def test_option_defaults_are_the_librarys():
    """DEFAULTS above is what the library starts with (the other tests restore options from it)."""
    for name, value in DEFAULTS.items():
        assert _lib.lib().emg3d_get_option(name.encode()) == value, name


# ------------------------------------------------------------------------------------------- A
# (shape, inside?): interior nodes and thread slots hx hy (nz - 1) of the kernel's stride loop (rounds of 256)
SMALL_SHAPES = [((9, 9, 9), True),       # 512 nodes, 200 slots: the last shape that is in, one round
                ((10, 9, 9), False),     # 576 nodes: out -- the option must be inert
                ((65, 3, 5), True),      # 512 nodes, 264 slots: second round, long x
                ((33, 3, 9), True),      # 512 nodes, 272 slots
                ((3, 5, 65), True),      # 512 nodes, 384 slots: second round, long z
                ((2, 2, 2), True),       # one interior node
                ((3, 2, 2), True)]       # two
VARIANTS = [(complex, False), (float, False), (complex, True)]
# sweeps per call: 5 is the first with more than 16 passes (the upper half of the word), 8 fills all 64 bits when no
# pass is skipped, 9 (36 passes) must fall back to one launch per colour
NUS = (1, 2, 4, 5, 8, 9)


def _nodes(shape):
    return (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)


def _slots(shape):
    return ((shape[0] + 1) // 2) * ((shape[1] + 1) // 2) * (shape[2] - 1)


def test_small_shapes_are_what_the_table_says():
    assert [(_nodes(s), _slots(s)) for s, _ in SMALL_SHAPES] == [(512, 200), (576, 200), (512, 264), (512, 272),
                                                                (512, 384), (1, 1), (2, 2)]
    assert all((_nodes(s) <= DEFAULTS['point_small']) == inside for s, inside in SMALL_SHAPES)
    assert 4 * 8 <= 32 < 4 * 9      # (the launcher's limit: 4 nu <= 32 passes)


def _small_case(shape, dtype, extras):
    grid, vm, rng = random_level(shape, 'triaxial', dtype, 17 * sum(shape) + 3 * int(extras) + int(dtype is float),
                                 extras=extras)
    if extras:      # (eta has a real part in every cell: the eta sums are stored in full)
        assert all(np.all(eta.real != 0) for eta in (vm.eta_x, vm.eta_y, vm.eta_z))
    return grid, vm, rng


def _oracle_point(vm, grid, s, e0, nu):
    a = e0.copy()
    ocore.gauss_seidel(a.fx, a.fy, a.fz, s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h, nu, order=1)
    assert np.all(np.isfinite(a.field))
    return a.field


@pytest.mark.parametrize('dtype,extras', VARIANTS, ids=['complex', 'real', 'complex-extras'])
@pytest.mark.parametrize('shape,inside', SMALL_SHAPES, ids=['x'.join(map(str, s)) for s, _ in SMALL_SHAPES])
def test_point_small_equals_launch_per_colour_and_oracle(shape, inside, dtype, extras):
    """core.gauss_seidel (the host wrapper: eta sums from emg3d_dev_point_setup) with point_small = 512 and 0, for
    nu = 1, 2, 4, 5, 8, 9 x point_order 0 / 1 x skip_repeat 0 / 1: the same device function in the same pass order on
    the same sums, so the same bits; and the one-launch result against the oracle in that order, rel-L2 < 1e-10 (the
    tolerance of test_randomised_smoother_parity; the smoother contracts, so it does not grow with nu)."""
    lib, olib = _lib.lib(), ocore.lib()
    grid, vm, rng = _small_case(shape, dtype, extras)
    s, e0 = random_field(grid, dtype, rng), random_field(grid, dtype, rng, pec=True)
    worst = {}
    try:
        for order in (0, 1):
            _set('point_order', order)
            olib.oracle_set_point_repeat(order)
            for nu in NUS:
                want = _oracle_point(vm, grid, s, e0, nu)
                for skip in (0, 1):
                    _set('skip_repeat', skip)
                    got = {}
                    for small in (512, 0):
                        _set('point_small', small)
                        b = e0.copy()
                        core.gauss_seidel(b.fx, b.fy, b.fz, s.fx, s.fy, s.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta,
                                          *grid.h, nu)
                        got[small] = b.field.copy()
                    at = (shape, dtype.__name__, extras, order, nu, skip)
                    assert np.any(got[512] != e0.field), at
                    assert np.array_equal(got[512], got[0]), (at, relerr(got[512], got[0]))
                    d = relerr(got[512], want)
                    worst[nu] = max(worst.get(nu, 0.0), d)
                    assert d < 1e-10, (at, d)
    finally:
        _restore_defaults()
    print(f"\nA oracle-distance {'x'.join(map(str, shape))} {dtype.__name__}{' extras' if extras else ''} inside={inside}: "
          + ' '.join(f"nu={nu}:{d:.2e}" for nu, d in sorted(worst.items())))


def _device_sweeps(lv, s, e0, nu, sums):
    """nu point sweeps on a DeviceLevel from (s, e0) (host vectors, one per right-hand side stacked): with the stored
    eta sums (DeviceLevel.smooth) or without (fac = NULL: the kernel forms them on the fly)."""
    lv.s.copy_(torch.from_numpy(s))
    lv.e.copy_(torch.from_numpy(e0))
    if sums:
        lv.smooth(0, nu)
    else:
        _lib.check(_lib.lib().emg3d_dev_gauss_seidel(lv._cref, 0, nu, None, None, None, 0, _stream()),
                   'emg3d_dev_gauss_seidel')
    return lv.e.cpu().numpy()


@pytest.mark.parametrize('dtype', [complex, float])
@pytest.mark.parametrize('shape', [s for s, inside in SMALL_SHAPES if inside], ids=lambda s: 'x'.join(map(str, s)))
def test_point_small_without_stored_sums(shape, dtype):
    """The same comparison for the variant without stored eta sums (emg3d_dev_gauss_seidel with fac = NULL on a
    DeviceLevel): point_small = 512 against 0 bit for bit, and against the oracle (1e-10)."""
    lib, olib = _lib.lib(), ocore.lib()
    grid, vm, rng = _small_case(shape, dtype, False)
    s, e0 = random_field(grid, dtype, rng), random_field(grid, dtype, rng, pec=True)
    lv = DeviceLevel.from_host(vm, torch.device('cuda'))
    worst = {}
    try:
        for order in (0, 1):
            _set('point_order', order)
            olib.oracle_set_point_repeat(order)
            for nu in NUS:
                want = _oracle_point(vm, grid, s, e0, nu)
                for skip in (0, 1):
                    _set('skip_repeat', skip)
                    got = {}
                    for small in (512, 0):
                        _set('point_small', small)
                        got[small] = _device_sweeps(lv, s.field, e0.field, nu, sums=False)
                    at = (shape, dtype.__name__, order, nu, skip)
                    assert np.any(got[512] != e0.field), at
                    assert np.array_equal(got[512], got[0]), (at, relerr(got[512], got[0]))
                    d = relerr(got[512], want)
                    worst[nu] = max(worst.get(nu, 0.0), d)
                    assert d < 1e-10, (at, d)
    finally:
        _restore_defaults()
    print(f"\nA oracle-distance (no sums) {'x'.join(map(str, shape))} {dtype.__name__}: "
          + ' '.join(f"nu={nu}:{d:.2e}" for nu, d in sorted(worst.items())))


@pytest.mark.parametrize('dtype', [complex, float])
def test_point_small_single_source_equals_its_slot_in_a_batch(dtype):
    """A level of three right-hand sides on (9, 9, 9) takes the launch-per-colour path (the one-workgroup kernel serves
    batch == 1): every source gets the bits of its own single-source call, which takes the one-launch path -- with and
    without stored sums, for every sweep count."""
    shape = (9, 9, 9)
    grid, vm, rng = _small_case(shape, dtype, False)
    dev = torch.device('cuda')
    srcs = [random_field(grid, dtype, rng).field for _ in range(3)]
    starts = [random_field(grid, dtype, rng, pec=True).field for _ in range(3)]
    n = grid.n_edges
    try:
        _restore_defaults()
        one, many = DeviceLevel.from_host(vm, dev), DeviceLevel.from_host(vm, dev, batch=3)
        for nu in NUS:
            for sums in (True, False):
                got = _device_sweeps(many, np.concatenate(srcs), np.concatenate(starts), nu, sums).reshape(3, n)
                for b in range(3):
                    want = _device_sweeps(one, srcs[b], starts[b], nu, sums)
                    assert np.any(want != starts[b])
                    assert np.array_equal(got[b], want), (dtype.__name__, nu, sums, b, relerr(got[b], want))
    finally:
        _restore_defaults()


# ------------------------------------------------------------------------------------------- B, C
@pytest.fixture(scope='module')
def problem():
    """The model of test_line_factor_policy_rebuild_equals_resident: (32, 24, 40) cells, stretched, random tri-axial
    resistivities; one dipole, and two more for the batches."""
    shape = (32, 24, 40)
    rng = np.random.default_rng(3)
    h = [widths(n // 2, n // 4, 30., 1.1) for n in shape]
    grid = emg3d.TensorMesh(h, [-w.sum() / 2 for w in h])
    rho = 10 ** rng.uniform(-0.5, 1.0, shape)
    model = emg3d.Model(grid, rho, 1.5 * rho, 2.5 * rho)
    sfields = [emg3d.get_source_field(grid, src, 0.8) for src in ((3., -2., 1., 20., 30.), (-40., 25., -10., 110., -15.),
                                                                  (60., 10., 30., -70., 50.))]
    return model, sfields, emg3d.models.VolumeModel(model, sfields[0])


def _levels(lv, seen=None):
    """Every level of the tree below (and including) lv, once."""
    seen = {} if seen is None else seen
    if id(lv) not in seen:
        seen[id(lv)] = lv
        for link in lv.children.values():
            _levels(link['level'], seen)
    return list(seen.values())


def _captured(hier):
    """Captured graphs below the top level."""
    return [entry for lv in _levels(hier.top)[1:] for entry in lv.__dict__.get('_graphs', {}).values()
            if entry['graph'] is not None]


def _run(problem, hier, batch, kw):
    """One solve (or batch) on `hier`: [(field, it_mg, exit_message, error_at_cycle)] per source."""
    model, sfields, _ = problem
    if batch:
        out = solver.solve_batch(model, sfields, hierarchy=hier, **kw)
    else:
        out = [emg3d.solve(model, sfields[0], return_info=True, hierarchy=hier, **kw)]
    return [(e.field.copy(), info['it_mg'], info['exit_message'], np.array(info['error_at_cycle'])) for e, info in out]


def _same(a, b):
    return all(np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2] and np.array_equal(x[3], y[3])
               for x, y in zip(a, b)) and len(a) == len(b)


# tol / maxit: every (sc_dir, lr_dir) variant of the direction cycling (period 3) recurs at least four times -- two eager
# occurrences, the capture with its replay, another replay -- which takes 12 cycles (the oracle's F-cycle reaches 1e-11 of
# the source's norm after 14 cycles on this model); asserted below on the graphs and replays themselves
SOLVE = dict(sslsolver=False, tol=1e-13, maxit=14)
REPLAY_CONFIGS = {
    'defaults': dict(),
    'direct-form': dict(residual_form=False),
    'F-cycle': dict(cycle='F'),
    'point-only': dict(semicoarsening=False, linerelaxation=False),
    'residual-form': dict(residual_form=True),
    'line-compact': dict(_line_compact=True),
    'fp64-records': dict(_line_compact=False),
    'omega-1.2': dict(smoother_omega=1.2),
    'krylov-V': dict(sslsolver=True, cycle='V'),
    'batch': dict(_batch=True),
    'batch-residual-form': dict(_batch=True, residual_form=True),
}


@pytest.mark.parametrize('name', list(REPLAY_CONFIGS))
def test_replayed_coarse_correction_equals_eager(problem, name, monkeypatch):
    """Each kind of solve twice on fresh hierarchies: with _cycle.USE_GRAPHS off (every coarse-grid correction launched
    eagerly) and as shipped (two eager occurrences of a variant, then captured and replayed). Fields, cycle counts,
    exit messages and error histories must be equal bit for bit: a replay with stale operands -- a factor buffer, a
    scratch address, a direction of another variant -- would change them."""
    kw = dict(SOLVE, **REPLAY_CONFIGS[name])
    batch, compact = kw.pop('_batch', False), kw.pop('_line_compact', None)
    vmodel = problem[2]
    replays = {'n': 0}
    orig = torch.cuda.CUDAGraph.replay

    def counting_replay(self):
        replays['n'] += 1
        return orig(self)
    monkeypatch.setattr(torch.cuda.CUDAGraph, 'replay', counting_replay)
    out, hiers = {}, {}
    try:
        _restore_defaults()
        for graphs in (False, True):
            monkeypatch.setattr(_cycle, 'USE_GRAPHS', graphs)
            hier = hiers[graphs] = solver.Hierarchy(vmodel, batch=3 if batch else 1, line_compact=compact)
            out[graphs] = _run(problem, hier, batch, kw)
            if not graphs:
                assert replays['n'] == 0 and not _captured(hier)
    finally:
        _restore_defaults()
    captured = _captured(hiers[True])
    print(f"\nB {name}: {len(captured)} graphs captured, {replays['n']} replays, it_mg {[o[1] for o in out[True]]}, "
          f"{out[True][0][2]}")
    variants = 3 if kw.get('semicoarsening', True) else 1
    assert len(captured) >= variants and replays['n'] >= 2 * len(captured), (len(captured), replays['n'])
    if compact:
        lib = _lib.lib()
        assert any(lib.emg3d_line_compact_used(lv._cref, lr) for lv in _levels(hiers[True].top)[1:] for lr in (1, 2, 3))
    assert _same(out[False], out[True]), [(relerr(a[0], b[0]), a[1:3], b[1:3]) for a, b in zip(out[False], out[True])]


@pytest.mark.parametrize('tree', ['one-tree', 'semicoarsened'])
@pytest.mark.parametrize('policy', ['resident', 'rebuild', 'single'])
def test_second_solve_replays_from_its_first_cycle(problem, policy, tree, monkeypatch):
    """A second solve on the same hierarchy replays every coarse-grid correction from its first cycle on, behind
    another predecessor than the graph was captured behind: the first solve ends, after 14 cycles, on the second
    variant of the direction schedule, the capture of the first variant followed the third. Both solves against an
    eager one on a fresh hierarchy, bit for bit.

    'one-tree' (semicoarsening=False, line relaxation cycling through the codes 4, 5, 6) is where that matters for the
    policies 'rebuild' / 'single': ONE chain of coarse levels meets all three codes, so which directions a level's one
    or two factor buffers hold depends on the cycle before -- unless every correction starts without factors
    (Workspace.factor_epoch), a captured slot hit is stale when the graph is replayed behind another cycle. With
    semicoarsening ('semicoarsened') the code advances together with the semicoarsening direction, every direction
    has its own subtree, and a coarse level only ever sees one code: that case checks the replay, not the epoch."""
    vmodel = problem[2]
    kw = dict(SOLVE, semicoarsening=False) if tree == 'one-tree' else dict(SOLVE)
    replays = {'n': 0}
    orig = torch.cuda.CUDAGraph.replay

    def counting_replay(self):
        replays['n'] += 1
        return orig(self)
    monkeypatch.setattr(torch.cuda.CUDAGraph, 'replay', counting_replay)
    try:
        _restore_defaults()
        monkeypatch.setattr(_cycle, 'USE_GRAPHS', False)
        eager = _run(problem, solver.Hierarchy(vmodel, line_factors=policy), False, kw)
        monkeypatch.setattr(_cycle, 'USE_GRAPHS', True)
        hier = solver.Hierarchy(vmodel, line_factors=policy)
        first = _run(problem, hier, False, kw)
        assert first[0][1] % 3 != 0, first[0][1]      # (the next solve's first variant follows another one than at capture)
        assert len(_captured(hier)) == 3
        if tree == 'one-tree':
            assert len([lv for lv in _levels(hier.top)[1:] if '_graphs' in lv.__dict__]) == 1
        before = replays['n']
        second = _run(problem, hier, False, kw)
        assert replays['n'] - before == second[0][1] == first[0][1]       # (every cycle of the second solve replayed)
    finally:
        _restore_defaults()
    assert _same(first, eager), (policy, tree, relerr(first[0][0], eager[0][0]), first[0][1:3], eager[0][1:3])
    assert _same(second, eager), (policy, tree, relerr(second[0][0], eager[0][0]), second[0][1:3], eager[0][1:3])


# (option, value, (R): changes results?, solve keywords)
POINT_ONLY = dict(linerelaxation=False)
OPTION_CHANGES = {
    'point_small-0': ([('point_small', 0)], False, POINT_ONLY),
    'skip_repeat-0': ([('skip_repeat', 0)], False, {}),
    'line_fuse-0': ([('line_fuse', 0)], False, {}),
    'line_lds-0': ([('line_lds', 0)], False, {}),
    'line_lpw-8': ([('line_lpw', 8)], False, {}),
    'residual_zb-1': ([('residual_zb', 1)], False, {}),
    'line_order-0': ([('line_order', 0)], True, {}),
    'line_wide-0': ([('line_wide', 0)], True, {}),
    'point_order-0': ([('point_order', 0)], True, POINT_ONLY),
    'point_tile_min-1': ([('point_tile_min', 1)], True, POINT_ONLY),
    'point_tile_min-1+point_compact-1': ([('point_tile_min', 1), ('point_compact', 1)], True, POINT_ONLY),
    'line_compact-1': ([('line_compact', 1)], True, {}),
}
POLICIES = ('resident', 'rebuild')


def _check_caches(hier):
    """What _purge_stale_graphs and _drop_stale_factors promise after a solve: no graph of another option set is left
    anywhere in the tree, and no level keeps more than one eta-sum buffer."""
    now = _lib.options_fingerprint()
    for lv in _levels(hier.top):
        stale = [k for k in lv.__dict__.get('_graphs', {}) if k[-1] != now]
        assert not stale, (lv.grid.shape_cells, len(stale))
        points = [k for k in lv._factors if isinstance(k, tuple) and k[0] == 'point']
        assert len(points) <= 1, (lv.grid.shape_cells, points)


FORMAT_OPTIONS = {'line_compact': 'line', 'point_compact': 'point'}


def _record_formats(hier):
    """Per level: the bytes of the line records of the three directions and of the eta sums under the current options."""
    lib = _lib.lib()
    return [{'line': tuple(lib.emg3d_line_fac_bytes_lv(lv._cref, lr) for lr in (1, 2, 3)),
             'point': (lib.emg3d_point_compact_used(lv._cref), lib.emg3d_point_fac_bytes_lv(lv._cref))}
            for lv in _levels(hier.top)]


@pytest.fixture(scope='module')
def reused(problem):
    """One hierarchy per factor policy for all option changes, with the results of its solves under the defaults (line
    relaxation, and point smoothing only). The levels are not flagged for compact records (line_compact=False), so that
    every record is fp64 until an option says otherwise."""
    vmodel = problem[2]
    out = {}
    try:
        _restore_defaults()
        for policy in POLICIES:
            hier = solver.Hierarchy(vmodel, line_factors=policy, line_compact=False)
            first = {key: _run(problem, hier, False, dict(SOLVE, **kw)) for key, kw in (('lines', {}), ('points', POINT_ONLY))}
            _check_caches(hier)
            out[policy] = (hier, first)
    finally:
        _restore_defaults()
    yield out
    out.clear()


@pytest.mark.parametrize('change', list(OPTION_CHANGES))
@pytest.mark.parametrize('policy', POLICIES)
def test_reused_hierarchy_follows_changed_options(problem, reused, policy, change):
    """A hierarchy that has solved under the default options (fp64 records, graphs captured), then under changed ones,
    then under the defaults again: under the changed options it gives the bits of a fresh hierarchy -- and, for an
    option that include/emg3d_amd.h does not mark (R), the bits of the defaults --, and back under the defaults the
    bits of its first solve. The order default -> compact -> default only ever reads a larger buffer as a smaller
    format where a cache key misses an option (the opposite order writes past the end of a buffer)."""
    sets, changes_results, extra = OPTION_CHANGES[change]
    hier, first = reused[policy]
    kw = dict(SOLVE, **extra)
    e1 = first['points' if extra else 'lines']
    vmodel = problem[2]
    try:
        _restore_defaults()
        # (one hierarchy serves all cases: state that an earlier case left behind shows here, not under this case's option)
        base = _run(problem, hier, False, kw)
        assert _same(base, e1), (policy, change, 'before the change', relerr(base[0][0], e1[0][0]))
        for i, (name, value) in enumerate(sets):
            before = _record_formats(hier)
            _set(name, value)
            if name in FORMAT_OPTIONS:
                # the option really changes the size of a factor buffer on some level of this (unflagged) hierarchy
                which = FORMAT_OPTIONS[name]
                assert any(a[which] != b[which] for a, b in zip(before, _record_formats(hier))), (policy, change, name)
            if i == 0:
                # a solve that ends after one cycle visits one semicoarsening direction only: the graphs of the others
                # are stale all the same
                _run(problem, hier, False, dict(kw, maxit=1))
                _check_caches(hier)
            got = _run(problem, hier, False, kw)
            _check_caches(hier)
            want = _run(problem, solver.Hierarchy(vmodel, line_factors=policy, line_compact=False), False, kw)
            at = (policy, change, name)
            assert _same(got, want), (at, relerr(got[0][0], want[0][0]), got[0][1:3], want[0][1:3])
            if not changes_results:
                assert _same(got, e1), (at, relerr(got[0][0], e1[0][0]))
        _restore_defaults()
        again = _run(problem, hier, False, kw)
        _check_caches(hier)
        assert _same(again, e1), (policy, change, relerr(again[0][0], e1[0][0]), again[0][1:3], e1[0][1:3])
    finally:
        _restore_defaults()


@pytest.mark.parametrize('policy', POLICIES)
def test_reused_flagged_hierarchy_goes_back_to_fp64_records(problem, policy):
    """The other direction, compact -> fp64 -> compact, on a hierarchy whose levels ARE flagged for compact records
    (Hierarchy(line_compact=True)): line_fuse = 0 selects the separate launches, which read fp64 records only, so the
    z-lines of the 40-cell levels change their record format -- to larger buffers. Reused equals fresh under both."""
    vmodel, kw = problem[2], dict(SOLVE)
    lib = _lib.lib()
    try:
        _restore_defaults()
        hier = solver.Hierarchy(vmodel, line_factors=policy, line_compact=True)
        e1 = _run(problem, hier, False, kw)
        assert lib.emg3d_line_compact_used(hier.top._cref, 3) == 1
        _set('line_fuse', 0)
        assert lib.emg3d_line_compact_used(hier.top._cref, 3) == 0
        got = _run(problem, hier, False, kw)
        _check_caches(hier)
        want = _run(problem, solver.Hierarchy(vmodel, line_factors=policy, line_compact=True), False, kw)
        assert _same(got, want), (policy, relerr(got[0][0], want[0][0]), got[0][1:3], want[0][1:3])
        _restore_defaults()
        again = _run(problem, hier, False, kw)
        _check_caches(hier)
        assert _same(again, e1), (policy, relerr(again[0][0], e1[0][0]))
    finally:
        _restore_defaults()
