"""The BiCGSTAB loop of emg3d_amd/_krylov.py on the host: its control flow -- SciPy's iteration, breakdown codes and
stopping rule, and the per-source bookkeeping of a batch -- with the device replaced by the NumPy model of
tests/krylov_model.py (vector kernels, fill / copy, operator, preconditioner). No GPU: the kernels themselves are tested
in tests/test_krylov_kernels.py, the loop on the device in tests/test_gpu_parity.py.

Bounds: the iterates are compared with SciPy's own at 1e-12 (both run the same recurrence in float64 on a system of
condition ~1.5; they differ by the order of a few sums), true-residual histories at 1e-4 relative, which is meaningful
only while no iteration count hangs on rounding -- each comparison asserts that SciPy's last residual lies below
tol |b| and the one before it above.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

import krylov_model as km
from emg3d_amd import _device, _krylov

N, TOL, MAXIT, SEED = 40, 1e-10, 60, 34


def _system(is_complex=True):
    rng = np.random.default_rng(SEED)
    n1, n2 = rng.standard_normal((N, N)), rng.standard_normal((N, N))
    A = 4 * np.eye(N) + 0.12 * (n1 + 1j * n2 if is_complex else n1)
    B = rng.standard_normal((3, N)) + (1j * rng.standard_normal((3, N)) if is_complex else 0)
    B[1] *= 1e-3
    x0 = 0.1 * (rng.standard_normal(N) + (1j * rng.standard_normal(N) if is_complex else 0))
    return A, np.diag(1 / np.diag(A)), B, x0


A_C, M_C, B_C, X0_C = _system()
BREAK_A = np.array([[0., 1, 0, 0], [-1, 0, 0, 0], [0, 0, 3, 0], [0, 0, 0, 3]])
BREAK_B = np.array([[1., 0, 0, 0], [0, 0, 1, 1]])


def _scipy(A, b, tol, M=None, maxit=MAXIT, x0=None):
    """SciPy's solution, status and the true residual norm after every iteration (what its callback sees)."""
    hist = []
    x, code = spla.bicgstab(A, b, x0=x0, rtol=tol, atol=1e-30, maxiter=maxit, M=M,
                            callback=lambda xk: hist.append(np.linalg.norm(b - A @ xk)))
    return x, code, hist


def _install(monkeypatch):
    vectors, lib = km.vectors_class(), km.Lib()
    monkeypatch.setattr(_krylov, 'Vectors', vectors)
    for module in (_krylov, _device):
        monkeypatch.setattr(module, '_lib', lib)
        monkeypatch.setattr(module, '_stream', km.stream)
    return vectors


def _tensor(a, top):
    return torch.from_numpy(np.array(a, dtype=complex if top.is_complex else float).ravel())


def single(monkeypatch, A, M, b, tol=TOL, maxit=MAXIT, x0=None, run_cycles=None):
    """One right-hand side through ``_krylov.bicgstab``."""
    vectors = _install(monkeypatch)
    top = km.Top(A, M)
    var = SimpleNamespace(tol=tol, ssl_maxit=maxit, cycle='F' if M is not None else None)
    x, hist = _tensor(np.zeros(len(b)) if x0 is None else x0, top), []
    code = _krylov.bicgstab(SimpleNamespace(top=top), _tensor(b, top), x, var, run_cycles or top.run_cycles, hist.append)
    return SimpleNamespace(x=[x], code=[code], hist=[hist], top=top, vectors=vectors)


def batch(monkeypatch, A, M, B, tols=None, maxit=MAXIT, live=None, spoil=None):
    """The rows of ``B`` through ``_krylov.bicgstab_rows``, from a zero start. ``spoil`` = (call, source): the preconditioner
    fails for that source in its call number ``call`` (counted from 1) and clears its ``live`` flag."""
    vectors = _install(monkeypatch)
    nb = len(B)
    top = km.Top(A, M, nb)
    top.s.copy_(_tensor(B, top))
    tols = [TOL] * nb if tols is None else tols
    live = [True] * nb if live is None else live
    hist, calls = [[] for _ in range(nb)], []

    def precondition(SRC, OUT, live_now):
        calls.append([(v.steps, v.reads) for v in vectors.made])
        top.precondition_rows(SRC, OUT, live_now)
        if spoil is not None and len(calls) == spoil[0]:
            live_now[spoil[1]] = False

    X = torch.zeros_like(top.s)
    code = _krylov.bicgstab_rows(top, top.s.clone(), X, tols, maxit, precondition, lambda b, l2: hist[b].append(l2), live)
    return SimpleNamespace(x=top.rows(X), code=list(code), hist=hist, top=top, vectors=vectors, calls=calls, live=live)


def _fair(hist, b, tol):
    """The iteration count does not hang on rounding: SciPy's last residual is below tol |b|, the one before above."""
    bound = tol * np.linalg.norm(b)
    return hist[-1] < bound < hist[-2]


def _check_against_scipy(got, i, A, M, b, tol, x0=None):
    x, code, hist = _scipy(A, b, tol, M, x0=x0)
    assert _fair(hist, b, tol), (hist[-2:], tol * np.linalg.norm(b))
    assert got.code[i] == code == 0
    assert len(got.hist[i]) == len(hist)
    err = np.linalg.norm(got.x[i].numpy() - x) / np.linalg.norm(x)
    hist_err = np.max(np.abs(np.array(got.hist[i]) / np.array(hist) - 1))
    print(f"source {i}: {len(hist)} iterations, |x - x_scipy| / |x_scipy| = {err:.1e}, history within {hist_err:.1e}")
    assert err <= 1e-12
    assert hist_err <= 1e-4


# ----------------------------------------------------------------------------------------------- a. against SciPy
@pytest.mark.parametrize('i', range(3))
def test_single_matches_scipy(monkeypatch, i):
    got = single(monkeypatch, A_C, M_C, B_C[i])
    _check_against_scipy(got, 0, A_C, M_C, B_C[i], TOL)


def test_single_with_start_vector_matches_scipy(monkeypatch):
    got = single(monkeypatch, A_C, M_C, B_C[0], x0=X0_C)
    _check_against_scipy(got, 0, A_C, M_C, B_C[0], TOL, x0=X0_C)


def test_batch_matches_scipy(monkeypatch):
    got = batch(monkeypatch, A_C, M_C, B_C)
    for i in range(3):
        _check_against_scipy(got, i, A_C, M_C, B_C[i], TOL)


# --------------------------------------------------------------------------------- b. batch rows are single solves
@pytest.mark.parametrize('tols', [[TOL, TOL, TOL], [TOL, 1e-4, TOL]], ids=['same-tol', 'one-stops-early'])
def test_batch_rows_are_single_solves(monkeypatch, tols):
    got = batch(monkeypatch, A_C, M_C, B_C, tols=tols)
    for i, tol in enumerate(tols):
        one = single(monkeypatch, A_C, M_C, B_C[i], tol=tol)
        assert torch.equal(got.x[i], one.x[0])
        assert got.code[i] == one.code[0] == 0
        assert got.hist[i] == one.hist[0]
        assert len(one.hist[0]) == len(_scipy(A_C, B_C[i], tol, M_C)[2])
    counts = [len(h) for h in got.hist]
    assert counts[0] == counts[2] and (counts[1] < counts[0]) == (tols[1] > TOL)


# ---------------------------------------------------------------------------------------------------- c. breakdown
def test_breakdown_code_and_the_source_next_to_it(monkeypatch):
    """rt . v = 0 in the first iteration of source 0: SciPy's -11, x = 0, no callback -- and source 1 converges."""
    ref = [_scipy(BREAK_A, b, TOL) for b in BREAK_B]
    assert ref[0][1] == -11 and not ref[0][0].any() and ref[0][2] == [] and ref[1][1] == 0
    got = batch(monkeypatch, BREAK_A, None, BREAK_B)
    ones = [single(monkeypatch, BREAK_A, None, b) for b in BREAK_B]
    for i, (x, code, hist) in enumerate(ref):
        for res, k in ((got, i), (ones[i], 0)):
            assert res.code[k] == code
            assert len(res.hist[k]) == len(hist)
            assert np.allclose(res.x[k].numpy(), x, rtol=1e-12, atol=0)
        assert torch.equal(got.x[i], ones[i].x[0])
    assert got.live == [False, False]


# ---------------------------------------------------------------------------------------------- d. iteration limit
def test_iteration_limit(monkeypatch):
    A, M, B, _ = _system(is_complex=False)
    x, code, hist = _scipy(A, B[0], TOL, M, maxit=3)
    assert code == 3 and len(hist) == 3
    for got in (single(monkeypatch, A, M, B[0], maxit=3), batch(monkeypatch, A, M, B[:1], maxit=3)):
        assert got.code == [3] and len(got.hist[0]) == 3
        assert got.x[0].dtype == torch.float64
        assert np.linalg.norm(got.x[0].numpy() - x) / np.linalg.norm(x) <= 1e-12


# -------------------------------------------------------------------------------- e. a source not live at entry
def test_source_not_live_at_entry(monkeypatch):
    B = B_C.copy()
    B[1] = 0
    got = batch(monkeypatch, A_C, M_C, B, live=[True, False, True])
    assert not got.x[1].numpy().any() and got.hist[1] == []
    assert (got.vectors.made[1].steps, got.vectors.made[1].reads) == (0, 0)
    for i in (0, 2):
        one = single(monkeypatch, A_C, M_C, B_C[i])
        assert torch.equal(got.x[i], one.x[0]) and got.code[i] == 0 and got.hist[i] == one.hist[0]


# ------------------------------------------------------------------------------- f. a preconditioner that fails
def test_batch_source_whose_preconditioner_fails(monkeypatch):
    got = batch(monkeypatch, A_C, M_C, B_C, spoil=(2, 1))
    at_failure = got.calls[1][1]                   # (steps, reads) of source 1 when the second call began
    assert (got.vectors.made[1].steps, got.vectors.made[1].reads) == at_failure
    assert got.hist[1] == [] and got.live == [False] * 3
    for i in (0, 2):
        one = single(monkeypatch, A_C, M_C, B_C[i])
        assert torch.equal(got.x[i], one.x[0]) and got.code[i] == 0 and got.hist[i] == one.hist[0]


def test_single_preconditioner_error_propagates(monkeypatch):
    class Diverged(Exception):
        pass

    def run_cycles(top, var):
        raise Diverged("in the preconditioner")

    with pytest.raises(Diverged, match="in the preconditioner"):
        single(monkeypatch, A_C, M_C, B_C[0], run_cycles=run_cycles)


# ------------------------------------------------------------------------------------- g. synchronising reads
def test_synchronising_reads(monkeypatch):
    one = single(monkeypatch, A_C, M_C, B_C[0])
    its = len(one.hist[0])
    assert km.synchronising_reads(one.top, one.vectors) == 1 + 2 * its
    got = batch(monkeypatch, A_C, M_C, B_C)
    assert [len(h) for h in got.hist] == [its] * 3
    assert km.synchronising_reads(got.top, got.vectors) <= 3 + (2 * 3 + 1) * its
