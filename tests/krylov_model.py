"""TEST INFRASTRUCTURE ONLY: host stand-ins for what the BiCGSTAB loop of emg3d_amd/_krylov.py touches on the device, so
that its control flow (breakdown codes, stopping rule, the per-source bookkeeping of a batch) runs without a GPU.

  Vectors   the interface of ``_krylov.Vectors`` (new, slot, copy, step, read with extra=, put) on torch CPU tensors, with
            NumPy arithmetic; counts its ``step`` and ``read`` calls. ``step`` in the order of csrc/krylov.h: y = sum coef * x
            (all terms read before y is written: y may alias a term), then the inner products with the new y, then the
            scalar program
  Lib       ``emg3d_dev_zero`` / ``emg3d_dev_copy`` as memset / memmove on host pointers
  Top       what the loop reads of a ``DeviceLevel``: a dense operator, a fixed preconditioner matrix, ``e`` / ``s``

Operator, preconditioner and inner products are evaluated one right-hand side at a time by plain NumPy reductions (no
BLAS call, whose summation order may depend on where a row begins): a row of a batch sees exactly the arithmetic of a
single solve, so the two can be compared bit for bit.
"""
import ctypes

import numpy as np
import torch

DIV, MUL, NEG, COPY = 0, 1, 2, 3


def matvec(A, x):
    """A x by one pairwise row reduction per entry, the same bits wherever x begins."""
    return (A * np.asarray(x)[None, :]).sum(axis=1)


class Lib:
    """``_lib`` of the modules under test: ``check`` and the fill / copy entry points, on host memory."""

    @staticmethod
    def check(status, name):
        assert status == 0, name

    def lib(self):
        return self

    @staticmethod
    def emg3d_dev_zero(ptr, nbytes, stream):
        ctypes.memset(ptr, 0, nbytes)
        return 0

    @staticmethod
    def emg3d_dev_copy(dst, src, nbytes, stream):
        ctypes.memmove(dst, src, nbytes)
        return 0


def stream():
    return None


def vectors_class():
    """A fresh ``Vectors`` class; ``cls.made`` lists its instances in the order of their creation."""

    class Vectors:
        NSLOTS = 32
        made = []                    # (one list per class: this function makes a new class for every solve)

        def __init__(self, top, n=None, nslots=None):
            self.top = top
            self.n = top.e.numel() if n is None else int(n)
            self.is_complex = top.is_complex
            if nslots is not None:
                self.NSLOTS = int(nslots)
            self.table = np.zeros(self.NSLOTS, dtype=complex if self.is_complex else float)
            self._names = {}
            self.steps = self.reads = self.reads_with_extra = 0
            type(self).made.append(self)

        def new(self):
            return torch.empty(self.n, dtype=self.top.dtype)

        def slot(self, name):
            if name not in self._names:
                self._names[name] = len(self._names)
                assert len(self._names) <= self.NSLOTS
            return self._names[name]

        def put(self, names, values):
            for nm, v in zip(names, values):
                self.table[self.slot(nm)] = v

        def copy(self, dst, src):
            dst.copy_(src)

        def step(self, y=None, terms=(), dots=(), prog=()):
            self.steps += 1
            t = self.table
            with np.errstate(all='ignore'):
                if terms:
                    acc = 0
                    for x, coef in terms:
                        assert x.numel() == self.n
                        if isinstance(coef, tuple):
                            c = t[self.slot(coef[0])] * float(coef[1])
                        elif isinstance(coef, str):
                            c = t[self.slot(coef)]
                        else:
                            c = float(coef)
                        acc = acc + c * x.numpy()
                    y.numpy()[:] = acc
                for name, a, b in dots:
                    t[self.slot(name)] = np.sum(np.conj(a.numpy()) * b.numpy())
                for op, dst, a, b in prog:
                    va = t[self.slot(a)]
                    vb = t[self.slot(b)] if b is not None else None
                    t[self.slot(dst)] = {DIV: lambda: va / vb, MUL: lambda: va * vb, NEG: lambda: -va,
                                         COPY: lambda: va}[op]()

        def read(self, *names, extra=None):
            self.reads += 1
            self.reads_with_extra += extra is not None
            out = [complex(self.table[self.slot(nm)]) if self.is_complex else float(self.table[self.slot(nm)])
                   for nm in names]
            return (out, extra.numpy().copy()) if extra is not None else out

    return Vectors


class Grid:
    def __init__(self, n):
        self.n_edges = n


class Top:
    """The finest level as the loop sees it: ``batch`` right-hand sides of ``A.shape[0]`` entries. ``M``: the fixed
    preconditioner matrix (None: identity)."""

    def __init__(self, A, M=None, batch=1):
        self.A, self.M = np.ascontiguousarray(A), M
        self.batch, self.grid = batch, Grid(A.shape[0])
        self.is_complex = np.iscomplexobj(A)
        self.dtype = torch.complex128 if self.is_complex else torch.float64
        self.device = torch.device('cpu')
        self.e, self.s = (torch.zeros(batch * A.shape[0], dtype=self.dtype) for _ in range(2))
        self.sumsq = torch.zeros(batch, dtype=torch.float64)
        self.sumsq_launches = 0

    def rows(self, t):
        n = self.grid.n_edges
        return [t[b * n:(b + 1) * n] for b in range(t.numel() // n)]

    def zero_field(self):
        self.e.zero_()

    def apply_A(self, x, out):
        for xr, outr in zip(self.rows(x), self.rows(out)):
            outr.numpy()[:] = matvec(self.A, xr.numpy())
        return out

    def residual_sumsq(self, x, b):
        self.sumsq_launches += 1
        for i, (xr, br) in enumerate(zip(self.rows(x), self.rows(b))):
            self.sumsq[i] = float(np.sum(np.abs(br.numpy() - matvec(self.A, xr.numpy())) ** 2))
        return self.sumsq

    def precondition_rows(self, src, out, which=None):
        """out <- M src for the rows ``which`` (all by default)."""
        for b, (sr, outr) in enumerate(zip(self.rows(src), self.rows(out))):
            if which is None or which[b]:
                outr.numpy()[:] = sr.numpy() if self.M is None else matvec(self.M, sr.numpy())

    def run_cycles(self, top, var):
        """``run_cycles`` of a single solve's preconditioner: e <- M s."""
        assert top is self and var.cycle
        self.precondition_rows(self.s, self.e)


def synchronising_reads(top, vectors):
    """Host reads that wait for the device: every ``Vectors.read``, and every true-residual sum that did not come
    along with one (``extra=``) and so was fetched by a copy of its own."""
    return (sum(v.reads for v in vectors.made) + top.sumsq_launches - sum(v.reads_with_extra for v in vectors.made))
