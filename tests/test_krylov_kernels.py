"""The vector kernels of the Krylov solvers (``csrc/krylov.h``) one call at a time: ``emg3d_dev_krylov_step`` (the fused
update ``k_kry_update`` and the reduction + scalar program ``k_kry_finish``), ``emg3d_dev_zero`` and ``emg3d_dev_copy``
against ``np.longdouble`` written out in this file, at the sizes where a path of the launch begins: a ragged wave, the
second workgroup, the second strided partial of the finish kernel (more than 256 workgroups), the capped grid (more
than 2048 workgroups of 256: a second and a third trip of the grid-stride loop).

Bounds (``EPS = 2**-52``), from the kernels' operation counts and not from what they were seen to give:

* dot, per real and imaginary part: ``(D + 4) EPS sum_i |a_i| |b_i|``, ``D = ceil(n / (G 256)) + 6 + 2 + ceil(G / 256) +
  8``, ``G = min(2048, max(1, ceil(n / 256)))``: serial accumulations of a thread, six shuffle levels, the sum over four
  waves, serial partials of a thread of the finish kernel, its eight tree levels; 4 for the roundings of one term.
* update, per element: ``4 (nterms + 1) EPS sum_k |c_k| |x_k,i|`` with ``c_k = table[slot] * scale`` as uploaded.
* scalar program: COPY and NEG exact, MUL ``4 EPS |a| |b|``, DIV ``8 EPS |a / b|`` in modulus for operands that are
  exact. An operand that this call computed (a dot, an earlier instruction) carries its own bound ``ea``, ``eb`` into
  the result by the triangle inequality, nothing else: ``|a' b' - a b| <= |a| eb + |b| ea + ea eb`` and
  ``|a' / b' - a / b| <= (ea + |a / b| eb) / (|b| - eb)``, plus the rounding of the instruction on the perturbed operands.

The reference sums in ``np.longdouble`` pairwise (``_psum``): its own error is ``(1 + log2 n) 2**-64`` of the same
sum of magnitudes, 1/200 of one EPS at the largest size. A dot with the updated ``y`` as an operand is taken with the
``y`` the device stored, downloaded again. Observed worst ratios of error to bound are printed and, with
``EMG3D_AMD_PARITY_FILE`` set, appended to that file (``profiles/krylov_kernels_parity.txt`` is such a run).
"""
import ctypes
import functools
import re
import types

import numpy as np
import pytest

from emg3d_amd import _lib
from test_sensitivity import record

EPS = 2.0 ** -52
NS = 16                                   # table slots of these tests
DIV, MUL, NEG, COPY = 0, 1, 2, 3          # include/emg3d_amd.h; the same as emg3d_amd._krylov (checked below)
_vp = ctypes.c_void_p

CAP = 2048 * 256                          # elements of one trip of the capped grid
SIZES = [1, 63, 64, 65, 255, 256, 257, 256 * 256, 256 * 256 + 1, 256 * 300 + 5, CAP - 1, CAP, CAP + 1, 2 * CAP + 257]
ODD_SIZES = [257, 256 * 256 + 1, CAP + 1]
KINDS = [True, False]                     # is_complex
ZERO_LENGTHS = [1, 255, 256, 257, 4096 * 256 - 1, 4096 * 256, 4096 * 256 + 1, 3 * 4096 * 256 + 77]


def _status(name):
    m = re.search(r'#define\s+%s\s+\((-?\d+)\)' % name, open(_lib.HEADER).read())
    return int(m.group(1))


def _addr(x):
    return x if x is None or isinstance(x, int) else x.data_ptr()


def _step(n, is_complex, table, y=None, terms=(), dots=(), prog=(), ws=None, ws_len=None, stream=None, nterms=None,
          ndots=None, nprog=None):
    """``emg3d_dev_krylov_step`` with raw addresses: ``terms`` [(x, slot, scale)], ``dots`` [(dslot, a, b)], ``prog``
    [(op, dst, a, b)] with slot numbers (b = -1: none); x, a, b, y, table, ws: tensors, integers or None. The counts
    can be overridden (the refusals). Returns the status."""
    nt, nd, npg = len(terms), len(dots), len(prog)
    xs = (_vp * max(nt, 1))(*[_addr(t[0]) for t in terms])
    slots = (ctypes.c_int * max(nt, 1))(*[t[1] for t in terms])
    scales = (ctypes.c_double * max(nt, 1))(*[t[2] for t in terms])
    das = (_vp * max(nd, 1))(*[_addr(d[1]) for d in dots])
    dbs = (_vp * max(nd, 1))(*[_addr(d[2]) for d in dots])
    dslots = (ctypes.c_int * max(nd, 1))(*[d[0] for d in dots])
    pr = (ctypes.c_int * max(4 * npg, 1))(*[v for ins in prog for v in ins])
    if ws_len is None:
        ws_len = 0 if ws is None else (ws.numel() if hasattr(ws, 'numel') else _lib.lib().emg3d_krylov_ws_len())
    return _lib.lib().emg3d_dev_krylov_step(
        n, int(is_complex), _addr(y), nt if nterms is None else nterms, xs, slots, scales, nd if ndots is None else ndots,
        das, dbs, dslots, npg if nprog is None else nprog, pr, _addr(table), _addr(ws), ws_len, stream)


# ----------------------------------------------------------------------- not gpu tests ---
FAKE = 0x10000                            # a non-null address: the refusals return before anything reads it


def _last_error():
    return (_lib.lib().emg3d_last_error() or b'').decode()


def test_instruction_codes_and_workspace_length():
    from emg3d_amd import _krylov
    assert (_krylov.DIV, _krylov.MUL, _krylov.NEG, _krylov.COPY) == (DIV, MUL, NEG, COPY)
    assert _lib.lib().emg3d_krylov_ws_len() >= 2048 * 3 * 2       # (re, im) of three dots for every workgroup


def test_krylov_step_refuses_bad_arguments():
    """Counts outside 0..4 terms, 0..3 dots, 0..8 instructions, no table, an update without ``y``: EMG3D_ERR_BADARG;
    dots without a workspace or with one that is a double short: EMG3D_ERR_SCRATCH. Nothing is launched."""
    badarg, scratch = _status('EMG3D_ERR_BADARG'), _status('EMG3D_ERR_SCRATCH')
    assert badarg != 0 and scratch != 0 and badarg != scratch
    full = _lib.lib().emg3d_krylov_ws_len()
    term, dot, ins = (FAKE, -1, 1.0), (0, FAKE, FAKE), (COPY, 1, 0, -1)
    good = dict(n=8, is_complex=1, table=FAKE, y=FAKE, terms=[term], dots=[dot], prog=[ins], ws=FAKE, ws_len=full)
    bad = [(badarg, dict(nterms=-1)), (badarg, dict(terms=[term] * 5)), (badarg, dict(dots=[dot] * 4)),
           (badarg, dict(prog=[ins] * 9)), (badarg, dict(table=None)), (badarg, dict(y=None)),
           (badarg, dict(y=None, dots=[], prog=[])),
           (scratch, dict(ws=None, ws_len=full)), (scratch, dict(ws_len=full - 1)),
           (scratch, dict(y=None, terms=[], ws=None)), (scratch, dict(y=None, terms=[], prog=[], ws_len=full - 1))]
    for code, kw in bad:
        for is_complex in (1, 0):
            _lib.lib().emg3d_set_option(b'no such option', 0)           # another message than the one expected below
            assert 'krylov_step' not in _last_error()
            assert _step(**{**good, 'is_complex': is_complex, **kw}) == code, kw
            assert 'krylov_step: ' in _last_error(), kw
            with pytest.raises(_lib.Emg3dAmdError, match='krylov_step: '):
                _lib.check(_step(**{**good, 'is_complex': is_complex, **kw}), 'emg3d_dev_krylov_step')


def test_zero_refuses_what_is_not_a_buffer_of_doubles():
    badarg = _status('EMG3D_ERR_BADARG')
    L = _lib.lib()
    for p, nbytes in ((FAKE, 12), (FAKE, 7), (FAKE, 8 * 1000 + 4), (FAKE + 4, 8), (FAKE + 1, 64), (FAKE + 12, 4)):
        L.emg3d_set_option(b'no such option', 0)
        assert 'zero: ' not in _last_error()
        assert L.emg3d_dev_zero(p, nbytes, None) == badarg, (p, nbytes)
        assert 'zero: ' in _last_error()


# ---------------------------------------------------------------- reference and checks ---
def _ld(v):
    return np.asarray(v).astype(np.clongdouble if np.iscomplexobj(v) else np.longdouble)


def _cld(re, im=0.0):
    z = np.zeros(1, dtype=np.clongdouble)
    z.real, z.imag = re, im
    return z[0]


def _psum(v):
    """Pairwise sum in the precision of ``v``: error (log2 n) ulp of the sum of magnitudes."""
    v = np.asarray(v)
    while v.size > 1:
        if v.size % 2:
            v = np.concatenate([v, np.zeros(1, dtype=v.dtype)])
        v = v[0::2] + v[1::2]
    return v[0]


def _reductions(n):
    """D of the module docstring, from n alone."""
    G = min(2048, max(1, -(-n // 256)))
    return -(-n // (G * 256)) + 6 + 2 + -(-G // 256) + 8


def _dot_ref(a, b):
    """conj(a) . b in extended precision and sum |a_i| |b_i|."""
    al, bl = _ld(a), _ld(b)
    return _cld(0) + _psum(np.conj(al) * bl), np.longdouble(_psum(np.abs(al) * np.abs(bl)))


def _coef(table, slot, scale, is_complex):
    s = np.longdouble(scale)
    if slot < 0:
        return s
    re = np.longdouble(table[2 * slot]) * s
    return _cld(re, np.longdouble(table[2 * slot + 1]) * s) if is_complex else re     # (real: the imaginary part is ignored)


def _check_update(got, table, terms, is_complex, what):
    """``got`` against sum c_k x_k; terms [(host x, slot, scale)]. Returns the worst error / bound."""
    exact, mag = 0, 0
    for x, slot, scale in terms:
        c = _coef(table, slot, scale, is_complex)
        exact, mag = exact + c * _ld(x), mag + np.abs(c) * np.abs(_ld(x))
    assert got.dtype == (np.complex128 if is_complex else np.float64) and got.shape == np.shape(exact)
    err, bound = np.abs(_ld(got) - exact), 4 * (len(terms) + 1) * EPS * mag
    assert np.all(np.isfinite(got)), what
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    assert np.all(err <= bound), (what, worst)
    return worst


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_table(got, table0, n, is_complex, dots, prog, what):
    """The table after a call against the one uploaded: ``dots`` [(dslot, host a, host b)] within the dot bound per
    part (real vectors: imaginary part exactly 0), ``prog`` re-run in extended precision with the bounds of the module
    docstring, every other slot bit-identical. Returns the worst error / bound of the dots."""
    assert np.all(np.isfinite(got)), (what, got)
    ratio = 0.0
    val = [_cld(table0[2 * s], table0[2 * s + 1]) for s in range(NS)]
    err = [np.longdouble(0)] * NS
    written = set()
    D = _reductions(n)
    for dslot, a, b in dots:
        exact, mag = _dot_ref(a, b)
        bound = (D + 4) * EPS * mag
        parts = [abs(np.longdouble(got[2 * dslot]) - exact.real), abs(np.longdouble(got[2 * dslot + 1]) - exact.imag)]
        worst = float(max(parts) / bound) if bound > 0 else (0.0 if max(parts) == 0 else np.inf)
        ratio = max(ratio, worst)
        assert parts[0] <= bound and parts[1] <= bound, (what, dslot, worst)
        if not is_complex or a is b:
            assert got[2 * dslot + 1] == 0.0, (what, dslot, got[2 * dslot + 1])
        val[dslot], err[dslot] = exact, bound * (np.sqrt(np.longdouble(2)) if is_complex else 1)
        written.add(dslot)
    for i, (op, dst, a, b) in enumerate(prog):
        assert not any(dst == d[0] for d in dots)              # (the dots above are compared after the program)
        va, ea = val[a], err[a]
        vb, eb = (val[b], err[b]) if b >= 0 else (_cld(1), np.longdouble(0))
        if op == DIV:
            assert abs(vb) > eb
            v = va / vb
            e = (ea + abs(v) * eb) / (abs(vb) - eb)
            e = e + 8 * EPS * (abs(v) + e)
        elif op == MUL:
            v = va * vb
            e = abs(va) * eb + abs(vb) * ea + ea * eb
            e = e + 4 * EPS * (abs(va) + ea) * (abs(vb) + eb)
        else:
            v, e = (-va if op == NEG else va), ea
        val[dst], err[dst] = v, e
        written.add(dst)
    for s in sorted(written - {d[0] for d in dots}):
        g = _cld(got[2 * s], got[2 * s + 1])
        assert abs(g - val[s]) <= err[s], (what, s, g, val[s], err[s])
    keep = np.array([s not in written for s in range(NS)]).repeat(2)
    assert np.array_equal(_bits(got)[keep], _bits(table0)[keep]), what
    return ratio


def _note(what, n, update=None, dot=None):
    """One line per test: the worst error / bound it saw."""
    parts = ([] if update is None else [f"update {update:.3f} (bound 4 (nterms + 1) EPS)"]) + \
            ([] if dot is None else [f"dot {dot:.2e} (bound (D + 4) EPS, D = {_reductions(n)})"])
    record(f"{what}: max |diff| / bound: " + ", ".join(parts))


def _ramp(n):
    return 10.0 ** np.linspace(-6.0, 6.0, n)


def _normal(n, is_complex, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n) if is_complex else rng.standard_normal(n)


@functools.lru_cache(maxsize=2)
def _operands(n, is_complex):
    """Five host vectors, each from its own seed, which no test changes: ``a`` scaled by a factor that runs from 1e-6 to
    1e+6 along the vector, ``b = (2 - 3j) a + noise`` (real: ``-3 a + noise``), so that conj(a) . b has the imaginary
    part -3 |a|^2, ``c`` scaled by the factor reversed, ``d`` and ``e`` plain; and the table: NS random (re, im) pairs."""
    seed = 7919 * n + 100 * is_complex
    a = _normal(n, is_complex, seed) * _ramp(n)
    b = ((2 - 3j) if is_complex else -3.0) * a + 0.25 * _normal(n, is_complex, seed + 1)
    c = _normal(n, is_complex, seed + 2) * _ramp(n)[::-1]
    d, e = _normal(n, is_complex, seed + 3), _normal(n, is_complex, seed + 4)
    table = np.random.default_rng(seed + 5).standard_normal(2 * NS)
    for v in (a, b, c, d, e, table):
        v.setflags(write=False)
    return (a, b, c, d, e), table


def _dev():
    import torch
    return torch.device('cuda', torch.cuda.current_device())


def _up(a):
    import torch
    return torch.from_numpy(np.array(a)).to(_dev())


@functools.lru_cache(maxsize=2)
def _device_operands(n, is_complex):
    """``_operands`` in device memory (a test that writes to one of them writes to a clone)."""
    return tuple(_up(v) for v in _operands(n, is_complex)[0])


def _workspace(value=float('nan')):
    import torch
    return torch.full((_lib.lib().emg3d_krylov_ws_len(),), value, dtype=torch.float64, device=_dev())


def _run(n, is_complex, table0, y=None, terms=(), dots=(), prog=()):
    """One call on the current stream with a fresh copy of ``table0`` and a workspace of NaN. Returns the table."""
    from emg3d_amd._device import _stream
    table, ws = _up(table0), _workspace()
    _lib.check(_step(n, is_complex, table, y, terms, dots, prog, ws, stream=_stream()), 'emg3d_dev_krylov_step')
    return table.cpu().numpy()


def _kind(is_complex):
    return 'complex' if is_complex else 'real'


# ---------------------------------------------------------------- krylov_step on the gpu ---
@pytest.mark.gpu
@pytest.mark.parametrize('alias', ['distinct', 'first', 'last'])
@pytest.mark.parametrize('is_complex', KINDS)
@pytest.mark.parametrize('n', SIZES)
def test_update_only(n, is_complex, alias):
    """``y = sum c_k x_k`` for one to four terms, ``y`` a vector of its own, ``x_0`` or the last ``x_k``; the form of
    the coefficient (bare scale, slot, slot and scale) moves along the terms from case to case. The table is unchanged."""
    host, table0 = _operands(n, is_complex)
    dev = _device_operands(n, is_complex)
    forms = [(-1, 0.75), (3, 1.0), (6, -1.5)]
    worst = 0.0
    for nterms in (1, 2, 3, 4):
        shift = nterms + ['distinct', 'first', 'last'].index(alias)
        coefs = [forms[(k + shift) % 3] for k in range(nterms)]
        xs = list(dev[:nterms])
        iy = {'distinct': None, 'first': 0, 'last': nterms - 1}[alias]
        y = dev[4].clone() if iy is None else xs[iy].clone()
        if iy is not None:
            xs[iy] = y
        got = _run(n, is_complex, table0, y, [(x, s, c) for x, (s, c) in zip(xs, coefs)])
        assert np.array_equal(_bits(got), _bits(table0))
        worst = max(worst, _check_update(y.cpu().numpy(), table0, [(x, s, c) for x, (s, c) in zip(host, coefs)],
                                         is_complex, f"n={n} {_kind(is_complex)} nterms={nterms} y={alias}"))
    _note(f"update only n={n} {_kind(is_complex)} y={alias}, nterms 1..4", n, update=worst)
    assert all(np.array_equal(_bits(d.cpu().numpy()), _bits(h)) for d, h in zip(dev, host))


@pytest.mark.gpu
@pytest.mark.parametrize('is_complex', KINDS)
@pytest.mark.parametrize('n', SIZES)
def test_dots_only(n, is_complex):
    """One, two and three inner products without an update, into slots that are not neighbours: ``a . a`` (imaginary
    part exactly 0), ``a . b`` with the imaginary part -3 |a|^2, ``c . d``."""
    (a, b, c, d, e), table0 = _operands(n, is_complex)
    da, db, dc, dd, de = _device_operands(n, is_complex)
    dots_dev, dots_host = [(11, da, da), (2, da, db), (5, dc, dd)], [(11, a, a), (2, a, b), (5, c, d)]
    assert all(table0[2 * s + 1] != 0 for s in (11, 2, 5))
    worst = 0.0
    for nd in (1, 2, 3):
        got = _run(n, is_complex, table0, dots=dots_dev[:nd])
        worst = max(worst, _check_table(got, table0, n, is_complex, dots_host[:nd], [],
                                        f"n={n} {_kind(is_complex)} ndots={nd}"))
    _note(f"dots only n={n} {_kind(is_complex)}, ndots 1..3", n, dot=worst)


SOLVER_STEPS = ['r -= alpha v', 'w -= a q', 'r = b - r']


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SOLVER_STEPS)
@pytest.mark.parametrize('is_complex', KINDS)
@pytest.mark.parametrize('n', SIZES)
def test_update_and_dots_in_one_call(n, is_complex, shape):
    """The fused steps of the solvers; the inner products are taken with the NEW ``y``, as operand a, b or both."""
    (a, b, c, d, e), table0 = _operands(n, is_complex)
    da, db, dc, dd, de = _device_operands(n, is_complex)
    if shape == 'r -= alpha v':                 # (r, r) and (rt, r)
        y, y0 = da.clone(), a
        terms, hterms = [(y, -1, 1.0), (dc, 3, 1.0)], [(a, -1, 1.0), (c, 3, 1.0)]
        dots = lambda v, vb, B: [(5, v, v), (9, B, v)]                 # noqa: E731
    elif shape == 'w -= a q':                   # (q', w), and the other way round
        y, y0 = da.clone(), a
        terms, hterms = [(y, -1, 1.0), (dd, 4, -1.0)], [(a, -1, 1.0), (d, 4, -1.0)]
        dots = lambda v, A, B: [(2, B, v), (7, v, B)]                  # noqa: E731
    else:                                       # (b, b) and (r, r); y is the LAST term
        y, y0 = dc.clone(), c
        terms, hterms = [(da, -1, 1.0), (y, -1, -1.0)], [(a, -1, 1.0), (c, -1, -1.0)]
        dots = lambda v, A, B: [(1, A, A), (6, v, v)]                  # noqa: E731
    what = f"'{shape}' n={n} {_kind(is_complex)}"
    got = _run(n, is_complex, table0, y, terms, dots(y, da, db))
    ynew = y.cpu().numpy()
    _note(what, n, update=_check_update(ynew, table0, hterms, is_complex, what),
          dot=_check_table(got, table0, n, is_complex, dots(ynew, a, b), [], what))


def _vectors(n, is_complex):
    """``_krylov.Vectors`` for vectors of n entries (what it reads of a level: dtype, device, is_complex)."""
    import torch
    from emg3d_amd import _krylov
    top = types.SimpleNamespace(is_complex=is_complex, device=_dev(), dtype=torch.complex128 if is_complex else torch.float64)
    V = _krylov.Vectors(top, n, nslots=NS)
    V.ws.fill_(float('nan'))
    return V


TAIL_NAMES = ['rho', 'alpha', 'omega', 'nomega', 'rr', 'rho_next', 'q1', 'q2', 'beta', 'bo', 'nbo']
TAIL = [(DIV, 'q1', 'rho_next', 'rho'), (DIV, 'q2', 'alpha', 'omega'), (MUL, 'beta', 'q1', 'q2'),
        (MUL, 'bo', 'beta', 'omega'), (NEG, 'nbo', 'bo', None), (COPY, 'rho', 'rho_next', None)]


def _tail_step(V, table0, r, t, rt):
    """The last step of a BiCGSTAB iteration (``_krylov.bicgstab``) through ``Vectors.step``. Returns the table, and
    dots and program with slot numbers."""
    for name in TAIL_NAMES:
        V.slot(name)
    V.table.copy_(_up(table0))
    V.step(r, [(r, 1.0), (t, 'nomega')], dots=[('rr', r, r), ('rho_next', rt, r)], prog=TAIL)
    prog = [(op, V.slot(dst), V.slot(a), -1 if b is None else V.slot(b)) for op, dst, a, b in TAIL]
    return V.table.cpu().numpy(), V.slot('nomega'), V.slot('rr'), V.slot('rho_next'), prog


@pytest.mark.gpu
@pytest.mark.parametrize('is_complex', KINDS)
@pytest.mark.parametrize('n', SIZES)
def test_bicgstab_tail(n, is_complex):
    """``r -= omega t``, ``(r, r)``, ``(rt, r)`` and the six instructions that make beta, -beta omega and the next rho
    of them: later instructions read this call's dots and earlier results. Every slot is compared."""
    (a, b, c, d, e), table0 = _operands(n, is_complex)
    da, db, dc, dd, de = _device_operands(n, is_complex)
    r = da.clone()
    got, nomega, rr, rho_next, prog = _tail_step(_vectors(n, is_complex), table0, r, dd, db)
    rnew = r.cpu().numpy()
    what = f"tail n={n} {_kind(is_complex)}"
    _note(what, n, update=_check_update(rnew, table0, [(a, -1, 1.0), (d, nomega, 1.0)], is_complex, what),
          dot=_check_table(got, table0, n, is_complex, [(rr, rnew, rnew), (rho_next, b, rnew)], prog, what))


@pytest.mark.gpu
@pytest.mark.parametrize('is_complex', KINDS)
def test_scalar_program(is_complex):
    """Programs without update and without dots (only ``k_kry_finish`` runs): each instruction alone, NEG and COPY
    to the bit, without a second operand where there is none, and eight instructions that feed one another."""
    table0 = _operands(257, is_complex)[1]
    t0 = table0.reshape(NS, 2)
    for op, b in ((DIV, 9), (MUL, 9), (NEG, -1), (COPY, -1), (DIV, -1), (MUL, -1), (DIV, 7), (MUL, 7)):
        got = _run(257, is_complex, table0, prog=[(op, 3, 7, b)])
        _check_table(got, table0, 257, is_complex, [], [(op, 3, 7, b)], f"program op={op} b={b} {_kind(is_complex)}")
        if op in (NEG, COPY):
            assert np.array_equal(_bits(got.reshape(NS, 2)[3]), _bits(-t0[7] if op == NEG else t0[7]))
    full = [(DIV, 0, 1, 2), (MUL, 3, 0, 4), (NEG, 5, 3, -1), (COPY, 6, 5, -1), (MUL, 7, 6, 6), (DIV, 8, 7, 1),
            (NEG, 9, 8, -1), (COPY, 1, 9, -1)]
    got = _run(257, is_complex, table0, prog=full)
    _check_table(got, table0, 257, is_complex, [], full, f"program of eight {_kind(is_complex)}")
    assert not np.array_equal(_bits(got.reshape(NS, 2)[1]), _bits(t0[1]))
    assert np.array_equal(_bits(_run(257, is_complex, table0)), _bits(table0))        # nothing at all to do


@pytest.mark.gpu
@pytest.mark.parametrize('is_complex', KINDS)
@pytest.mark.parametrize('n', SIZES)
def test_poisoned_workspace_and_repeat(n, is_complex):
    """A workspace full of NaN: finite results within the bounds, so every partial that is read was written by this
    call. The same call again (table and workspace as before it): the same bits in table and ``y``."""
    (a, b, c, d, e), table0 = _operands(n, is_complex)
    da, db, dc, dd, de = _device_operands(n, is_complex)
    what = f"poisoned n={n} {_kind(is_complex)}"
    res = []
    for _ in range(2):
        y = de.clone()
        got = _run(n, is_complex, table0, y, [(da, 6, 0.5), (dc, -1, 2.0)], [(0, y, y), (13, db, y), (8, y, dd)],
                   [(DIV, 10, 13, 0)])
        res.append((got, y.cpu().numpy()))
    ynew = res[0][1]
    _note(what, n, update=_check_update(ynew, table0, [(a, 6, 0.5), (c, -1, 2.0)], is_complex, what),
          dot=_check_table(res[0][0], table0, n, is_complex, [(0, ynew, ynew), (13, b, ynew), (8, ynew, d)],
                           [(DIV, 10, 13, 0)], what))
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])) and np.array_equal(_bits(res[0][1]), _bits(res[1][1]))


@pytest.mark.gpu
@pytest.mark.parametrize('is_complex', KINDS)
@pytest.mark.parametrize('n', ODD_SIZES)
def test_row_slices_of_one_allocation(n, is_complex):
    """Operands ``t[b n:(b + 1) n]`` with n odd, as ``bicgstab_rows`` passes them (a real row begins 8 bytes off a
    16-byte boundary): the BiCGSTAB tail on the middle row of three equals the stand-alone reference, the rows before
    and after it keep their bits."""
    import torch
    (a, b, c, d, e), table0 = _operands(n, is_complex)
    da, db, dc, dd, de = _device_operands(n, is_complex)
    rows = lambda t: t[n:2 * n]           # noqa: E731
    R, T, RT = torch.cat([dc, da, de]), torch.cat([de, dd, dc]), torch.cat([da, db, dd])
    T0, RT0 = T.clone(), RT.clone()
    got, nomega, rr, rho_next, prog = _tail_step(_vectors(n, is_complex), table0, rows(R), rows(T), rows(RT))
    assert torch.equal(T, T0) and torch.equal(RT, RT0)
    Rn = R.cpu().numpy()
    assert np.array_equal(_bits(Rn[:n]), _bits(c)) and np.array_equal(_bits(Rn[2 * n:]), _bits(e))
    rnew = Rn[n:2 * n]
    what = f"rows n={n} {_kind(is_complex)}"
    _note(what, n, update=_check_update(rnew, table0, [(a, -1, 1.0), (d, nomega, 1.0)], is_complex, what),
          dot=_check_table(got, table0, n, is_complex, [(rr, rnew, rnew), (rho_next, b, rnew)], prog, what))


# ------------------------------------------------------------ zero and copy on the gpu ---
SENTINEL = -1.2345e300


@pytest.mark.gpu
@pytest.mark.parametrize('n', ZERO_LENGTHS)
def test_zero_inside_a_larger_buffer(n):
    """n doubles that begin 8 bytes off a 16-byte boundary: all +0.0 afterwards, the doubles on both sides untouched;
    4096 * 256 is one trip of the kernel's capped grid."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    lo, hi = 5, 300
    buf = torch.full((lo + n + hi,), SENTINEL, dtype=torch.float64, device=_dev())
    _lib.check(_lib.lib().emg3d_dev_zero(_ptr(buf, lo), 0, _stream()), 'emg3d_dev_zero')
    assert bool((buf == SENTINEL).all())
    _lib.check(_lib.lib().emg3d_dev_zero(_ptr(buf, lo), 8 * n, _stream()), 'emg3d_dev_zero')
    assert bool((buf[lo:lo + n].view(torch.int64) == 0).all())
    assert bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + n:] == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize('is_complex', KINDS)
def test_copy_inside_a_larger_buffer(is_complex):
    import torch
    from emg3d_amd._device import _ptr, _stream
    n, lo, hi = 70001, 3, 300
    src = _up(_normal(n, is_complex, 11))
    src0 = src.clone()
    buf = torch.full((lo + n + hi,), SENTINEL, dtype=src.dtype, device=_dev())
    _lib.check(_lib.lib().emg3d_dev_copy(_ptr(buf, lo), _ptr(src), 0, _stream()), 'emg3d_dev_copy')
    assert bool((buf == SENTINEL).all())
    _lib.check(_lib.lib().emg3d_dev_copy(_ptr(buf, lo), _ptr(src), n * src.element_size(), _stream()), 'emg3d_dev_copy')
    words = lambda t: torch.view_as_real(t) if is_complex else t          # noqa: E731
    assert torch.equal(words(buf[lo:lo + n]).view(torch.int64), words(src0).view(torch.int64)) and torch.equal(src, src0)
    assert bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + n:] == SENTINEL).all())
