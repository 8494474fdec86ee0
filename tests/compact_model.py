"""TEST INFRASTRUCTURE ONLY: an independent NumPy model of one call of the line smoothers (gauss_seidel_x / _y / _z in the
kernels' colour order) with the records that correction levels keep in SINGLE precision -- each rounding site a named
switch. Independent of emg3d_amd/csrc/stencil.h in everything but the record LAYOUT:

  operator    assembled as a SciPy sparse matrix from the oracle's amat_x (r = s - A e) by probing with coloured unit
              vectors; a line's matrix is A[idx, idx], its right-hand side s[idx] - A[idx, rest] e
  line solve  the two-sided block elimination (top chain of standard blocks {E0(k), t(k+1)}, k = 0 .. m-1; bottom chain
              of mirrored blocks {E0(k), t(k)}, k = n0-1 .. m+2; middle block Q = {E0(m), t(m+1), E0(m+1)}; m =
              line_mid(n0)), written with generic dense blocks of A -- no knowledge of which entries are zero
  arithmetic  np.longdouble (default) or float64, vectorised over the lines of a colour class
  roundings   round_T          every stored T_k (and the 21 entries of T_Q) -> fp32; the chain carries unrounded factors
              round_w          every stored w_k -> fp32; the forward recurrence goes on with the unrounded value, the
                               middle and backward steps read the stored one
              round_middle_rhs r_Q -> fp32
              ("round": a cast through np.float32 / np.complex64)
  T records   the model's own inverses, or a buffer in the layout of emg3d_dev_line_setup (`fac_offset`)
"""
import numpy as np
import scipy.sparse as sp

from oracle import core as ocore
from oracle import mg_ref

STREAMED = dict(round_T=True, round_w=True, round_middle_rhs=True)     # k_line_stream<.., COMPACT>
THREE_PHASE = dict(round_T=True, round_w=False, round_middle_rhs=False)  # k_line_colour with compact T records
EXACT = dict(round_T=False, round_w=False, round_middle_rhs=False)


# ------------------------------------------------------------------------------------------- layout of the records
def line_pad(n0):
    return 2 if n0 <= 6 else 4


def line_mid(n0):
    return (n0 // 2) // line_pad(n0) * line_pad(n0)


def line_padded(n0):
    m, p = line_mid(n0), line_pad(n0)
    return m + 2 + (n0 - 2 - m + p - 1) // p * p


def class_counts(direction, shape, colour):
    """(cntp, cntq): lines of a colour class along the two transverse PHYSICAL node axes in memory order (p faster).
    colour = (p & 1) | ((q & 1) << 1); direction 0: (p, q) = (iy, iz), 1: (ix, iz), 2: (ix, iy)."""
    nx, ny, nz = shape
    npp, nq = (ny if direction == 0 else nx), (ny if direction == 2 else nz)

    def cnt(n, par):
        return n // 2 if par else (n - 1) // 2
    return cnt(npp, colour & 1), cnt(nq, (colour >> 1) & 1)


def fac_offset(direction, shape, colour, lid, block, entry):
    """Element offset of packed entry `entry` (T(r, m), m <= r, at r (r + 1) / 2 + m) of record `block` of line `lid`
    of colour class `colour` in the T buffer of emg3d_dev_line_setup: the classes one after the other, each block-major
    (record k of line lid at k * nlines + lid), n0p records per line. Arguments may be arrays."""
    n0p = line_padded(shape[direction])
    before = [0]
    for c in range(4):
        cp, cq = class_counts(direction, shape, c)
        before.append(before[-1] + cp * cq)
    cp, cq = class_counts(direction, shape, colour)
    return 15 * n0p * before[colour] + (np.asarray(block) * (cp * cq) + np.asarray(lid)) * 15 + np.asarray(entry)


def sweep_colours(nu):
    """Colour classes of the passes of a call of nu sweeps: the passes cycle through 1, 2, 3, 0, sweep `it` taking
    positions 3 it .. 3 it + 3; a pass that repeats the one before it reproduces its values and is left out."""
    seq, out = (1, 2, 3, 0), []
    for it in range(nu):
        for cc in range(4):
            c = seq[(3 * it + cc) & 3]
            if not (cc == 0 and out and out[-1] == c):
                out.append(c)
    return out


# --------------------------------------------------------------------------------------------------- the operator
def assemble(grid, vm, dtype):
    """A (SciPy CSR, n_edges x n_edges, field dtype) from amat_x by coloured probing: unit vectors on every third edge
    of a component in each direction -- the stencil reaches edges whose three indices differ by at most one."""
    dt = np.complex128 if dtype is complex else np.float64
    shapes = (grid.shape_edges_x, grid.shape_edges_y, grid.shape_edges_z)
    offs = np.r_[0, np.cumsum([int(np.prod(s)) for s in shapes])]
    lin = [offs[c] + np.arange(int(np.prod(shapes[c]))).reshape(shapes[c], order='F') for c in range(3)]
    rows, cols, vals = [], [], []
    for c in range(3):
        for a in range(3):
            for b in range(3):
                for g in range(3):
                    e, r = mg_ref.Field(grid, dtype=dt), mg_ref.Field(grid, dtype=dt)
                    (e.fx, e.fy, e.fz)[c][a::3, b::3, g::3] = 1
                    ocore.amat_x(r.fx, r.fy, r.fz, e.fx, e.fy, e.fz, vm.eta_x, vm.eta_y, vm.eta_z, vm.zeta, *grid.h)
                    for c2, ae in enumerate((r.fx, r.fy, r.fz)):
                        idx = np.nonzero(ae)
                        # the one probed edge whose indices are within one of the row's
                        cidx = tuple(i + (par - i + 1) % 3 - 1 for i, par in zip(idx, (a, b, g)))
                        assert all(np.all((i >= 0) & (i < n)) for i, n in zip(cidx, shapes[c]))
                        rows.append(lin[c2][idx])
                        cols.append(lin[c][cidx])
                        vals.append(-ae[idx])
    n = int(offs[-1])
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n), dtype=dt)
    A.sum_duplicates()
    return A


def _ell(A):
    """Rows of a CSR matrix padded to equal length: (cols, vals), padding column -1 / value 0."""
    nnz = np.diff(A.indptr)
    w = int(nnz.max())
    cols = np.full((A.shape[0], w), -1, dtype=np.int64)
    vals = np.zeros((A.shape[0], w), dtype=A.dtype)
    pos = np.arange(A.nnz) - np.repeat(A.indptr[:-1], nnz)
    row = np.repeat(np.arange(A.shape[0]), nnz)
    cols[row, pos] = A.indices
    vals[row, pos] = A.data
    return cols, vals


def _round32(a):
    cplx = np.iscomplexobj(a)
    return a.astype(np.complex64 if cplx else np.float32).astype(a.dtype)


def _inverse(S):
    """Batched inverse (.., n, n) by Gauss-Jordan elimination with partial pivoting, in the dtype of S (numpy.linalg
    has no extended precision)."""
    S = S.copy()
    n = S.shape[-1]
    inv = np.broadcast_to(np.eye(n, dtype=S.dtype), S.shape).copy()
    ar = np.arange(S.shape[0])
    for j in range(n):
        p = j + np.argmax(np.abs(S[:, j:, j]), axis=1)
        for M in (S, inv):
            tmp = M[ar, p].copy()
            M[ar, p] = M[ar, j]
            M[ar, j] = tmp
        piv = 1 / S[:, j, j]
        S[:, j] *= piv[:, None]
        inv[:, j] *= piv[:, None]
        for i in range(n):
            if i != j:
                f = S[:, i, j].copy()
                S[:, i] -= f[:, None] * S[:, j]
                inv[:, i] -= f[:, None] * inv[:, j]
    return inv


def _mv(M, v):
    return (M * v[:, None, :]).sum(-1)


class LineModel:
    """One level, one line direction (0 / 1 / 2 = x / y / z) and one field dtype."""

    def __init__(self, grid, vm, direction, dtype, A=None):
        self.grid, self.vm, self.dir = grid, vm, direction
        self.shape = tuple(grid.shape_cells)
        self.cplx = dtype is complex
        self.A = assemble(grid, vm, dtype) if A is None else A
        self.ecols, self.evals = _ell(self.A)
        self.n0 = self.shape[direction]
        self.m = line_mid(self.n0)
        assert self.n0 >= 8, "both chains must hold a block"
        self._classes, self._couplings, self._own = {}, {}, {}

    # ---- unknowns of the lines of a colour class
    def _gidx(self, c, i0, i1, i2):
        """Position in [fx|fy|fz] of component c (0 along the line, 1 / 2 the cyclically next axes) at the abstract
        index (i0, i1, i2) = (along the line, next axis, next but one)."""
        nx, ny, nz = self.shape
        d = self.dir
        x, y, z = ((i0, i1, i2), (i2, i0, i1), (i1, i2, i0))[d]
        phys = (c + d) % 3
        g = self.grid
        if phys == 0:
            return x + nx * (y + (ny + 1) * z)
        if phys == 1:
            return g.n_edges_x + x + (nx + 1) * (y + ny * z)
        return g.n_edges_x + g.n_edges_y + x + (nx + 1) * (y + (ny + 1) * z)

    def lines(self, colour):
        """(E0 (L, n0), t (L, n0, 4): positions of the unknowns; t[:, k] = the transverse edges at node k (k >= 1))."""
        if colour not in self._classes:
            cp, cq = class_counts(self.dir, self.shape, colour)
            tp, tq = np.meshgrid(np.arange(cp), np.arange(cq), indexing='ij')
            lid = (tp + cp * tq).ravel()
            order = np.argsort(lid)
            p = ((1 if colour & 1 else 2) + 2 * tp).ravel()[order]
            q = ((1 if (colour >> 1) & 1 else 2) + 2 * tq).ravel()[order]
            i1, i2 = ((q, p) if self.dir == 1 else (p, q))
            i1, i2 = i1[:, None], i2[:, None]
            k = np.arange(self.n0)[None, :]
            e0 = self._gidx(0, k, i1, i2)
            t = np.stack([self._gidx(1, k, i1 - 1, i2), self._gidx(1, k, i1, i2),
                          self._gidx(2, k, i1, i2 - 1), self._gidx(2, k, i1, i2)], axis=-1)
            owner = np.full(self.A.shape[0], -1, dtype=np.int64)
            ln = np.arange(e0.shape[0])
            owner[e0] = ln[:, None]
            owner[t[:, 1:]] = ln[:, None, None]
            self._classes[colour] = (e0, t, owner)
        return self._classes[colour]

    def std(self, colour, k):
        e0, t, _ = self.lines(colour)
        return np.concatenate([e0[:, k:k + 1], t[:, k + 1]], axis=1)

    def mir(self, colour, k):
        e0, t, _ = self.lines(colour)
        return np.concatenate([e0[:, k:k + 1], t[:, k]], axis=1)

    def mid(self, colour):
        e0, t, _ = self.lines(colour)
        m = self.m
        return np.concatenate([e0[:, m:m + 1], t[:, m + 1], e0[:, m + 1:m + 2]], axis=1)

    def line_unknowns(self, colour):
        """(L, 5 n0 - 4) positions of all unknowns of each line."""
        e0, t, _ = self.lines(colour)
        return np.concatenate([e0, t[:, 1:].reshape(e0.shape[0], -1)], axis=1)

    def block(self, rows, cols):
        """A[rows, cols] per line: (L, a), (L, b) -> (L, a, b), in the matrix's dtype."""
        ec, ev = self.ecols[rows], self.evals[rows]
        return ((ec[..., None] == cols[:, None, None, :]) * ev[..., None]).sum(2)

    def couplings(self, colour):
        """B[k] = A[std k, std k-1] (k = 1 .. m-1), U[k] = A[mir k, mir k+1] (k = m+2 .. n0-2), and the middle block's
        A[Q, std m-1], A[Q, mir m+2]."""
        if colour not in self._couplings:
            m, n0 = self.m, self.n0
            B = {k: self.block(self.std(colour, k), self.std(colour, k - 1)) for k in range(1, m)}
            U = {k: self.block(self.mir(colour, k), self.mir(colour, k + 1)) for k in range(m + 2, n0 - 1)}
            Q = self.mid(colour)
            self._couplings[colour] = (B, U, self.block(Q, self.std(colour, m - 1)), self.block(Q, self.mir(colour, m + 2)))
        return self._couplings[colour]

    # ---- T records
    def own_records(self, colour, wt):
        """The model's own inverses in working type wt: ({k: T_k (L, 5, 5)}, T_Q (L, 6, 6)), unrounded."""
        key = (colour, np.dtype(wt).name)
        if key not in self._own:
            m, n0 = self.m, self.n0
            B, U, QB, QU = (self._cast(x, wt) for x in self.couplings(colour))
            T = {}
            for k in range(m):
                s = self.std(colour, k)
                S = self.block(s, s).astype(wt)
                if k:
                    S = S - B[k] @ T[k - 1] @ np.swapaxes(B[k], 1, 2)
                T[k] = _inverse(S)
            for k in range(n0 - 1, m + 1, -1):
                s = self.mir(colour, k)
                S = self.block(s, s).astype(wt)
                if k < n0 - 1:
                    S = S - U[k] @ T[k + 1] @ np.swapaxes(U[k], 1, 2)
                T[k] = _inverse(S)
            q = self.mid(colour)
            S = self.block(q, q).astype(wt)
            S = S - QB @ T[m - 1] @ np.swapaxes(QB, 1, 2) - QU @ T[m + 2] @ np.swapaxes(QU, 1, 2)
            self._own[key] = (T, _inverse(S))
        return self._own[key]

    @staticmethod
    def _cast(x, wt):
        if isinstance(x, dict):
            return {k: v.astype(wt) for k, v in x.items()}
        return x.astype(wt)

    def buffer_records(self, colour, fac):
        """The records of a colour class from a buffer in the layout of emg3d_dev_line_setup (1-D array of any real or
        complex type), as full symmetric matrices in the buffer's dtype: ({k: (L, 5, 5)}, (L, 6, 6))."""
        e0 = self.lines(colour)[0]
        lid = np.arange(e0.shape[0])
        r5, c5 = np.tril_indices(5)
        T = {}
        for k in [*range(self.m), *range(self.m + 2, self.n0)]:
            off = fac_offset(self.dir, self.shape, colour, lid[:, None], k, np.arange(15)[None, :])
            M = np.zeros((lid.size, 5, 5), dtype=fac.dtype)
            M[:, r5, c5] = fac[off]
            M[:, c5, r5] = fac[off]
            T[k] = M
        r6, c6 = np.tril_indices(6)
        a = fac[fac_offset(self.dir, self.shape, colour, lid[:, None], self.m, np.arange(15)[None, :])]
        b = fac[fac_offset(self.dir, self.shape, colour, lid[:, None], self.m + 1, np.arange(6)[None, :])]
        pk = np.concatenate([a, b], axis=1)
        TQ = np.zeros((lid.size, 6, 6), dtype=fac.dtype)
        TQ[:, r6, c6] = pk
        TQ[:, c6, r6] = pk
        return T, TQ

    # ---- one colour pass
    def rhs(self, colour, pos, e, s, wt):
        """s[pos] - A[pos, rest] e, rest = everything but the line's own unknowns; pos (L, a)."""
        owner = self.lines(colour)[2]
        out = np.empty(pos.shape, dtype=wt)
        step = max(1, 4_000_000 // (pos.shape[1] * self.ecols.shape[1]))
        for a in range(0, pos.shape[0], step):
            p = pos[a:a + step]
            ec = self.ecols[p]
            outside = owner[ec] != np.arange(a, a + p.shape[0])[:, None, None]      # (padding: value 0 anyway)
            out[a:a + step] = s[p] - (self.evals[p].astype(wt) * e[ec] * outside).sum(-1)
        return out

    def colour_pass(self, colour, e, s, wt, records=None, round_T=False, round_w=False, round_middle_rhs=False,
                    trace=None):
        """Solve all lines of a colour class and write the solution into e (working type wt, in place).
        records: (T, TQ) to use as stored (None: the model's own, rounded when stored if round_T).
        trace: dict that receives 'w' (L, blocks, 5): the stored w records, and 'x' (L, 5 n0 - 4)."""
        m, n0 = self.m, self.n0
        if records is None:
            T, TQ = self.own_records(colour, wt)
            if round_T:
                T, TQ = {k: _round32(v) for k, v in T.items()}, _round32(TQ)
        else:
            T, TQ = self._cast(records[0], wt), records[1].astype(wt)
        B, U, QB, QU = (self._cast(x, wt) for x in self.couplings(colour))
        rnd = _round32 if round_w else (lambda a: a)
        # all right-hand sides of the pass at once; columns as in line_unknowns: E0(k) at k, t(k) at n0 + 4 (k - 1) ..
        rall = self.rhs(colour, self.line_unknowns(colour), e, s, wt)
        four = np.arange(4)

        def r_std(k):
            return np.concatenate([rall[:, k:k + 1], rall[:, n0 + 4 * k + four]], axis=1)

        def r_mir(k):
            return np.concatenate([rall[:, k:k + 1], rall[:, n0 + 4 * (k - 1) + four]], axis=1)
        stored = {}
        w = None
        for k in range(m):                                    # top: w_k = T_k (r_k - B_k w_{k-1})
            c = r_std(k)
            if k:
                c = c - _mv(B[k], w)
            w = _mv(T[k], c)
            stored[k] = rnd(w)
        for k in range(n0 - 1, m + 1, -1):                    # bottom: w_k = T_k (r'_k - U_k w_{k+1})
            c = r_mir(k)
            if k < n0 - 1:
                c = c - _mv(U[k], w)
            w = _mv(T[k], c)
            stored[k] = rnd(w)
        rq = np.concatenate([r_std(m), rall[:, m + 1:m + 2]], axis=1)
        if round_middle_rhs:
            rq = _round32(rq)
        xq = _mv(TQ, rq - _mv(QB, stored[m - 1]) - _mv(QU, stored[m + 2]))
        sol = {}
        x = _mv(np.swapaxes(QB, 1, 2), xq)                    # coupling of the block behind to the one solved last
        for k in range(m - 1, -1, -1):                        # top: x_k = w_k - T_k B_{k+1}^T x_{k+1}
            xk = stored[k] - _mv(T[k], x)
            sol[k] = xk
            if k:
                x = _mv(np.swapaxes(B[k], 1, 2), xk)
        x = _mv(np.swapaxes(QU, 1, 2), xq)
        for k in range(m + 2, n0):                            # bottom: x_k = w_k - T_k U_{k-1}^T x_{k-1}
            xk = stored[k] - _mv(T[k], x)
            sol[k] = xk
            if k < n0 - 1:
                x = _mv(np.swapaxes(U[k], 1, 2), xk)
        for k in range(m):
            e[self.std(colour, k)] = sol[k]
        for k in range(m + 2, n0):
            e[self.mir(colour, k)] = sol[k]
        e[self.mid(colour)] = xq
        if trace is not None:
            trace['w'] = np.stack([stored[k] for k in sorted(stored)], axis=1)
            trace['x'] = e[self.line_unknowns(colour)]
            trace['xq'] = xq

    def smooth(self, e0, s, nu, fac=None, longdouble=True, traces=None, **switches):
        """nu sweeps from field e0 with source s (1-D [fx|fy|fz]); returns the field in the working type.
        fac: T buffer in the layout of emg3d_dev_line_setup to take the stored records from (None: the model's own).
        traces: list that receives (colour, trace dict) per pass."""
        wt = ((np.clongdouble if longdouble else np.complex128) if self.cplx else
              (np.longdouble if longdouble else np.float64))
        e, s = e0.astype(wt), s.astype(wt)
        for colour in sweep_colours(nu):
            rec = None if fac is None else self.buffer_records(colour, fac)
            tr = None if traces is None else {}
            self.colour_pass(colour, e, s, wt, records=rec, trace=tr, **switches)
            if traces is not None:
                traces.append((colour, tr))
        return e


def line_distance(model, x, xm):
    """delta_line = max |x - x_m| / max |x_m| over the unknowns of each line, all four colour classes one after the
    other (class 0 first): 1-D array of (nx'-1)(ny'-1) values."""
    out = []
    for colour in range(4):
        pos = model.line_unknowns(colour)
        a, b = x[pos], xm[pos]
        out.append((np.abs(a - b).max(1) / np.abs(b).max(1)).astype(np.float64))
    return np.concatenate(out)


# ------------------------------------------------------------------------------- cases, thresholds, the criterion
def line_offsets(model):
    """First global line number of each colour class (classes one after the other, class 0 first) and the total."""
    n = [model.line_unknowns(c).shape[0] for c in range(4)]
    return np.r_[0, np.cumsum(n)]


def random_level(shape, lr, dtype, seed=None, freq=0.7, extras=False):
    """Level of the compact-record tests: random widths stretched 2 % per cell away from the centre, random tri-axial
    conductivities over two decades at `freq` Hz (complex) or s = freq (real), random source and start field (zero on
    the PEC faces); extras: with epsilon_r and mu_r (at MHz eta gets a real part). Returns (grid, vm, s, e0) of the
    oracle's types."""
    rng = np.random.default_rng(sum(shape) + lr if seed is None else seed)
    h = [rng.uniform(5., 15., n) * 1.02 ** np.abs(np.arange(n) - n // 2) for n in shape]
    grid = mg_ref.Grid(h, (0., 0., 0.))
    sig = [10 ** rng.uniform(-1, 1, shape) for _ in range(3)]
    kw = dict(mu_r=rng.uniform(0.8, 2.0, shape), epsilon_r=rng.uniform(1., 80., shape)) if extras else {}
    vm = mg_ref.volume_model(grid, freq if dtype is complex else -abs(freq), *sig, **kw)
    s, e0 = mg_ref.Field(grid, dtype=dtype), mg_ref.Field(grid, dtype=dtype)
    for f in (s, e0):
        f.field[:] = rng.standard_normal(f.field.size)
        if dtype is complex:
            f.field[:] += 1j * rng.standard_normal(f.field.size)
    for v in (e0.fx[:, 0, :], e0.fx[:, -1, :], e0.fx[:, :, 0], e0.fx[:, :, -1], e0.fy[0], e0.fy[-1],
              e0.fy[:, :, 0], e0.fy[:, :, -1], e0.fz[0], e0.fz[-1], e0.fz[:, 0], e0.fz[:, -1]):
        v[...] = 0
    return grid, vm, s, e0


def pass_distance(model, colour, x, xm):
    """delta_line over the unknowns of the lines of one colour class (fields x, x_m)."""
    pos = model.line_unknowns(colour)
    return (np.abs(x[pos] - xm[pos]).max(1) / np.abs(xm[pos]).max(1)).astype(np.float64)


class Expectation:
    """What the model says about one level with given stored records `fac`, and the per-line criterion.

    First sweep, pass by pass (every line once), three evaluations of each pass from the SAME state -- that of the
    longdouble build with `switches`:
      tau     the float64 build with the same stored records: delta_line to the longdouble build, maximum over the
              lines whose stored w records agree, times 10 (summation order of the kernels: fused multiply-adds,
              two-stage sums);
      d_line  the model without any rounding (its own longdouble inverses): what the single-precision records change.
    The criterion for a result x with model value x_m: delta_line <= tau, but for the lines where two fp64 evaluations
    of a w entry fall on either side of an fp32 rounding boundary -- at most `cap` of the lines, none beyond d_line.

    A flipped line's neighbours read its values in the next pass and leave tau too (a flip is worth 1e-8, tau 1e-12):
    followed through a whole call from the start field, one flip in the first pass reaches every line within nine
    passes. The criterion is therefore applied where both sides solve from the same state: `compare_last_pass` (the
    lines of the last pass of a call saw exactly the final field around them) and, for the CPU walk, pass by pass.
    `compare` is the whole-call form: exact for records without flips (w kept in fp64), a figure otherwise."""

    def __init__(self, model, e0, s, fac, switches):
        self.model, self.switches, self.fac = model, dict(switches), fac
        self.e0, self.s = e0, s
        wt = self.wt = np.clongdouble if model.cplx else np.longdouble
        w64 = np.complex128 if model.cplx else np.float64
        e, sl = e0.astype(wt), s.astype(wt)
        off = line_offsets(model)
        spread, flipped, d_line = np.zeros(off[-1]), np.zeros(off[-1], bool), np.zeros(off[-1])
        for c in sweep_colours(1):
            rec = model.buffer_records(c, fac)
            e64, x, ta, tb = e.astype(w64), e.copy(), {}, {}
            model.colour_pass(c, e64, s.astype(w64), w64, records=rec, trace=ta, **self.switches)
            model.colour_pass(c, x, sl, wt, **EXACT)
            model.colour_pass(c, e, sl, wt, records=rec, trace=tb, **self.switches)
            spread[off[c]:off[c + 1]] = pass_distance(model, c, e64, e)
            d_line[off[c]:off[c + 1]] = pass_distance(model, c, x, e)
            if self.switches['round_w']:
                flipped[off[c]:off[c + 1]] = (ta['w'] != tb['w'].astype(w64)).any(axis=(1, 2))
        self.spread, self.flipped, self.d_line = spread, flipped, d_line
        self.tau = 10 * float(spread[~flipped].max())
        self._fields = {1: e}

    def tau_is_tight(self):
        """One missing fp32 rounding is never inside tau."""
        return self.tau <= 1e-3 * float(np.median(self.d_line))

    def field(self, nu):
        """The model's field after the call of nu sweeps from the start field (longdouble build)."""
        if nu not in self._fields:
            n0 = max(k for k in self._fields if k < nu)
            e, sl = self._fields[n0].copy(), self.s.astype(self.wt)
            for c in sweep_colours(nu)[len(sweep_colours(n0)):]:
                self.model.colour_pass(c, e, sl, self.wt, records=self.model.buffer_records(c, self.fac), **self.switches)
            self._fields[nu] = e
        return self._fields[nu]

    def compare(self, x, nu):
        """Whole call: (share of the lines above tau, worst delta_line / d_line, |x - x_m| / |x_m| in the 2-norm)."""
        xm = self.field(nu)
        d = line_distance(self.model, x, xm)
        return (float((d > self.tau).mean()), float((d / self.d_line).max()),
                float(np.linalg.norm((x - xm).astype(np.complex128)) / np.linalg.norm(xm.astype(np.complex128))))

    def compare_pass(self, x, c):
        """The lines of colour class c in a field x whose last pass solved that class, the model's pass taken from x
        itself (a line's right-hand side does not hold its own unknowns). Returns (lines above tau, of them beyond
        their d_line of this pass, lines of the pass, worst delta_line / d_line)."""
        model, wt = self.model, self.wt
        a, b, sl = x.astype(wt), x.astype(wt), self.s.astype(wt)
        model.colour_pass(c, a, sl, wt, records=model.buffer_records(c, self.fac), **self.switches)
        model.colour_pass(c, b, sl, wt, **EXACT)
        d, dl = pass_distance(model, c, x, a), pass_distance(model, c, b, a)
        return int((d > self.tau).sum()), int(((d > self.tau) & (d > dl)).sum()), d.size, float((d / dl).max())

    def compare_last_pass(self, x, nu):
        """compare_pass for the result x of a call of nu sweeps: nu = 1, 2, 3, 4 end with the classes 0, 3, 2, 1."""
        return self.compare_pass(x, sweep_colours(nu)[-1])


def record_errors(model, fac):
    """Stored single-precision records `fac` (layout of emg3d_dev_line_setup) against the model's own longdouble
    inverses T. An entry may be off by half its fp32 spacing (a correct rounding) plus what two fp64 factorisations
    differ by: 10 x the float64-vs-longdouble spread of the model's own records of that block (largest over the lines
    of the class, relative to the record's largest entry). Returns (worst |stored - T| less that allowance, in units of
    the entry's fp32 spacing: at most 0.5; worst relative distance of a whole record)."""
    wt = np.clongdouble if model.cplx else np.longdouble
    w64 = np.complex128 if model.cplx else np.float64
    worst, rel = 0.0, 0.0
    for c in range(4):
        T, TQ = model.own_records(c, wt)
        D, DQ = model.own_records(c, w64)
        S, SQ = model.buffer_records(c, fac)
        for k in [*T, 'Q']:
            t, d, st = (TQ, DQ, SQ) if k == 'Q' else (T[k], D[k], S[k])
            size = np.abs(t).max(axis=(1, 2)).astype(np.float64)
            allow = 10 * float((np.abs(d - t).max(axis=(1, 2)) / size).max()) * size[:, None, None]
            for part in ((np.real, np.imag) if model.cplx else (np.asarray,)):
                err = np.abs(part(st).astype(np.float64) - part(t).astype(np.float64)) - allow
                ulp = np.spacing(np.abs(part(st)).astype(np.float32)).astype(np.float64)
                worst = max(worst, float((err / ulp).max()))
            rel = max(rel, float((np.abs(st - t).max(axis=(1, 2)) / size).max()))
    return worst, rel
