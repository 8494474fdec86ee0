"""Passes over the kept fields of ``gradient.ReciprocalSensitivity`` for a block of K columns, the
block PCG of ``gauss_newton_solve`` on top of them and the orthonormalisation of a device block
(DESIGN.md 4.21). Host code: every kernel is an entry point of the library; between the kernels of a pass the host
queues torch operations on (K, ns, nr) and waits for nothing."""
import types

import numpy as np
import torch

from emg3d_amd import _lib
from emg3d_amd._device import _ptr, _stream, free_hbm


def _call(name, *args):
    """The entry point ``name`` of the library on the current stream; raises unless it returns 0."""
    _lib.check(getattr(_lib.lib(), name)(*args, _stream()), name)


class _BlockPass:
    """K columns through the kept fields of ``rec`` in groups of at most ``kc``, frequency by frequency. The object
    owns the scratch of its products: each buffer is allocated when a product first needs it and used again by every
    later one (all run on one stream, in order), so that a kept pass allocates nothing after its first products. One
    product at a time: ``grad`` and the results of ``dots`` belong to the pass, the next product overwrites them.

    The primitives are ``stage`` (a frequency's two stacks in HBM), ``dots`` and ``combine``; the four products are
    ``jvec``, ``jtvec``, ``hessian_vec`` and ``precondition``. Uploads (``keep='host'``: a frequency's stacks; the
    coefficients of ``jtvec``) and the look at the free HBM come before a frequency's first kernel. ``expand``: the
    rows of a block that the three conductivity components read; ``weights``: the checked data weights of
    ``hessian_vec``, which its first product uploads."""

    def __init__(self, rec, dev, K, kc, expand, weights=None):
        self.rec, self.dev, self.K, self.kc, self.expand = rec, dev, K, min(kc, K), expand
        self.weights, self.wdevs = weights, None         # frequency name -> device (ns, nr), where a weight is not 0
        self.freqs = list(rec._per_frequency())
        stride = max(f[3].n_edges for f in self.freqs)
        self.stride = stride + (stride & 1)              # rows of float64 on 16-byte boundaries
        self.wbuf = None                                 # (kc, stride) edge weights
        self.tbufs = {}                                  # field type -> (kc, stride) edge vectors
        self.grad = None                                 # (K, 3, n_cells) cell gradients
        self.ws, self.res = {}, {}                       # frequency name -> workspace of dots_block, its (K, ns, nr)
        self.d = self.y = self.fws = None                # the stacked data (K, M) around the filter, its workspace

    def _scratch(self, dtype, what):
        """(kc, stride) of ``dtype`` in HBM for the columns of a group; raises if that much is not free."""
        rows = self.kc
        need = rows * self.stride * torch.empty(0, dtype=dtype).element_size()
        free = free_hbm(self.dev)
        if need > free:                                  # (one column, as for jvec / jtvec: nothing smaller to advise)
            raise MemoryError(f"ReciprocalSensitivity: the {what} of {rows} columns per pass need {need:,} B of HBM, "
                              f"{free:,} B are free" + ("; a smaller `columns_per_pass` needs less." if rows > 1 else "."))
        return torch.empty((rows, self.stride), dtype=dtype, device=self.dev)

    # ------------------------------------------------------------------------- primitives ---
    def stage(self, freq, combine=True):
        """The entry ``freq`` of ``freqs`` with its two stacks in HBM (ONE ``_fields_of``), whether they are complex
        and the type of its edge vectors, whose scratch ``combine`` needs."""
        fname, mine, gkey, grid, vol, plan, smu0 = freq
        estack, xstack = self.rec._fields_of(fname)
        is_complex = int(estack.is_complex())
        ftype = torch.complex128 if is_complex else torch.float64
        if combine and ftype not in self.tbufs:          # (before the kernels: the look at the free HBM is a host call)
            self.tbufs[ftype] = self._scratch(ftype, 'edge vectors')
        return types.SimpleNamespace(fname=fname, gkey=gkey, grid=grid, vol=vol, plan=plan, smu0=smu0, estack=estack,
                                     xstack=xstack, is_complex=is_complex, ftype=ftype, sp=self.rec._sp(estack))

    def dots(self, f, cells):
        """J of the staged frequency ``f`` times the block ``cells`` (K, n, n_cells) on its grid: one
        ``emg3d_dev_edge_weights`` per column and one ``emg3d_dev_sensitivity_dots_block`` per group -> (K, ns, nr)."""
        K, kc, wbuf, E, X = self.K, self.kc, self.wbuf, f.estack, f.xstack
        nx, ny, nz = f.grid.shape_cells
        n, o1, o2 = f.grid.n_edges, f.grid.n_edges_x, f.grid.n_edges_x + f.grid.n_edges_y
        ns, nr = len(E), len(X)
        # unit residual at a receiver: point source of strength conj(1 / (-s mu0)), times -s mu0 as every source
        # (residual_source_field) = kappa p_r; jvec = p_r^T A^-1 (-s mu0 w e_s) = -s mu0 / kappa sum w e_s x_r
        kappa = np.conj(1.0 / -f.smu0) * -f.smu0
        scale = complex(-f.smu0 / kappa)
        ws_len = _lib.lib().emg3d_sensitivity_dots_block_ws_len(ns, nr, kc, n)
        if f.fname not in self.ws:
            self.ws[f.fname] = torch.empty(ws_len, dtype=torch.float64, device=self.dev)
            self.res[f.fname] = torch.empty((K, ns, nr), dtype=f.ftype, device=self.dev)
        ws, res = self.ws[f.fname], self.res[f.fname]
        for g0 in range(0, K, kc):
            g1 = min(g0 + kc, K)
            for j in range(g0, g1):
                vx, vy, vz = (cells[j, k] for k in self.expand)
                w = wbuf[j - g0]
                _call('emg3d_dev_edge_weights', nx, ny, nz, _ptr(f.vol), _ptr(vx), _ptr(vy), _ptr(vz), _ptr(w), _ptr(w, o1),
                      _ptr(w, o2))
            _call('emg3d_dev_sensitivity_dots_block' + f.sp, n, f.is_complex, _ptr(E), E.stride(0), ns, _ptr(X), X.stride(0),
                  nr, _ptr(wbuf), self.stride, g1 - g0, scale.real, scale.imag, _ptr(res, g0 * ns * nr), _ptr(ws), ws_len)
        return res

    def combine(self, f, coef, active):
        """J^T of the staged frequency ``f`` for the columns ``active`` with the device coefficients ``coef`` (K, ns,
        nr), added to ``grad``: one ``emg3d_dev_sensitivity_combine_block`` per group and one
        ``emg3d_dev_edges_to_cells`` per column."""
        E, X, smu0 = f.estack, f.xstack, f.smu0
        nx, ny, nz = f.grid.shape_cells
        n, o1, o2 = f.grid.n_edges, f.grid.n_edges_x, f.grid.n_edges_x + f.grid.n_edges_y
        tbuf = self.tbufs[f.ftype]
        for g0 in range(0, len(active), self.kc):
            cols = active[g0:g0 + self.kc]
            # the coefficients of the group, contiguous (columns that are left out make gaps)
            cg = coef[cols[0]:cols[-1] + 1] if cols[-1] - cols[0] + 1 == len(cols) else coef[cols].contiguous()
            _call('emg3d_dev_sensitivity_combine_block' + f.sp, n, f.is_complex, _ptr(E), E.stride(0), len(E), _ptr(X),
                  X.stride(0), len(X), _ptr(cg), len(cols), _ptr(tbuf), self.stride)
            for row, j in enumerate(cols):
                t = tbuf[row]

                def to_cells(gtarget, nc):
                    _call('emg3d_dev_edges_to_cells', nx, ny, nz, f.is_complex, _ptr(t), _ptr(t, o1), _ptr(t, o2), smu0.real,
                          smu0.imag, _ptr(f.vol), _ptr(gtarget), _ptr(gtarget, nc), _ptr(gtarget, 2 * nc))
                self.rec._on_model_grid(f.plan, f.grid, self.grad[j], to_cells)

    def _on_grids(self, block):
        """The start of a product of the device block ``block``: the derivative chain of the mapping for the whole
        block, vector_k * d sigma / d property_k; returns ``cells(f)``, the block on the grid of a staged frequency --
        regridded once per product and grid."""
        if self.wbuf is None:
            self.wbuf = self._scratch(torch.float64, 'edge weights')
        on_model = block * self.rec._chain_factors(self.dev)
        regridded = {0: on_model}

        def cells(f):
            if f.gkey not in regridded:          # linear volume average: the map whose adjoint is the way back
                regridded[f.gkey] = torch.stack([torch.stack([f.plan.on_device(c, log=False) for c in col])
                                                 for col in on_model])
            return regridded[f.gkey]
        return cells

    def _zero_grad(self):
        if self.grad is not None:
            return self.grad.zero_()
        self.grad = torch.zeros((self.K, 3, self.rec.model.grid.n_cells), dtype=torch.float64, device=self.dev)
        return self.grad

    def shrink(self, K):
        """Fewer columns from now on (the block of a subspace method has lost rank), for ``jvec``, ``jtvec`` and
        ``hessian_vec``: the first K rows of ``grad`` and of the results of ``dots``; the scratch of a group stays as it
        is. The buffers of ``precondition`` (``d``, ``y``, ``fws``) are sized by the K of their first use and are not
        covered: a pass that has applied the preconditioner is not shrunk."""
        assert self.d is None and K <= self.K
        self.K = K
        self.grad = None if self.grad is None else self.grad[:K]
        self.res = {fname: res[:K] for fname, res in self.res.items()}

    # --------------------------------------------------------------------------- products ---
    def jvec(self, block):
        """J v for the K columns of the device block: dict frequency name -> device tensor (K, ns, nr)."""
        cells = self._on_grids(block)
        jv = {}
        for freq in self.freqs:
            f = self.stage(freq, combine=False)
            jv[f.fname] = self.dots(f, cells(f))
        return jv

    def jtvec(self, data):
        """J^T y for a list of K data dictionaries -> ``grad``. Coefficients: ``conj``, 0 for NaN or a missing pair,
        uploaded before the frequency's first kernel; columns without a datum at a frequency are left out there, a
        frequency without any is skipped."""
        rec, K, nrec = self.rec, self.K, len(self.rec._rec[0])
        grad = self._zero_grad()
        for freq in self.freqs:
            mine = freq[1]
            coef = np.zeros((K, len(mine), nrec), dtype=complex)
            for k, vector in enumerate(data):
                for row, i in enumerate(mine):
                    y = vector.get(rec.pairs[i])
                    if y is not None:
                        coef[k, row] = np.conj(np.nan_to_num(np.asarray(y, dtype=complex), nan=0.0))
            active = [k for k in range(K) if coef[k].any()]
            if active:
                f = self.stage(freq)
                cdev = torch.from_numpy(coef if f.is_complex else np.ascontiguousarray(coef.real)).to(self.dev)
                self.combine(f, cdev, active)
        return grad

    def hessian_vec(self, block):
        """J^T W J v for the K columns of the device block and the weights of the pass -> ``grad``; the coefficients
        ``conj(weights * jv)`` are formed on the device. A frequency whose weights are all zero is skipped, as in
        ``hessian_diagonal``."""
        cells = self._on_grids(block)
        grad = self._zero_grad()
        if self.wdevs is None:
            # every frequency's weights go up BEFORE the first kernel (an upload from pageable memory waits for the
            # stream): between dots_block and combine_block there are only torch operations on (K, ns, nr)
            self.wdevs = {}
            for fname, mine, *_ in self.freqs:
                wf = np.stack([self.weights[self.rec.pairs[i]] for i in mine])
                if wf.any():
                    self.wdevs[fname] = torch.from_numpy(np.ascontiguousarray(wf)).to(self.dev)
        for freq in self.freqs:
            if freq[0] in self.wdevs:
                f = self.stage(freq)
                jv = self.dots(f, cells(f))
                self.combine(f, torch.conj_physical(jv * self.wdevs[f.fname]).contiguous(), list(range(self.K)))
        return grad

    def precondition(self, block, pre, table):
        """The data-space half of the data preconditioner (``pre``: the dict of ``_data_preconditioner_setup``;
        ``table``: the PCG table of the running columns) between the two halves of a pass, in another order: ALL
        frequencies' ``dots`` first, their results gathered into the stacked real block (K, M) of ``stack_data`` by
        torch index operations on those small tensors, ONE ``emg3d_dev_data_space_filter`` on it, then all frequencies'
        ``combine`` with the coefficients ``conj`` of the filtered block, scattered back on the device -> ``grad``.
        ``keep='host'`` uploads each frequency's stacks TWICE, once for each half."""
        K, M, rank, index = self.K, pre['n_data'], pre['rank'], pre['index']
        cells = self._on_grids(block)
        grad = self._zero_grad()
        live = [freq for freq in self.freqs if freq[0] in index]      # (a frequency whose weights are all zero has s = 0)
        if self.d is None:
            self.d, self.y = (torch.zeros((K, M), dtype=torch.float64, device=self.dev) for _ in range(2))
        fws_len = _lib.lib().emg3d_data_space_filter_ws_len(rank, K)
        if self.fws is None:
            self.fws = torch.empty(fws_len, dtype=torch.float64, device=self.dev)
        d, y, jv = self.d, self.y, {}
        for freq in live:
            f = self.stage(freq)
            jv[f.fname] = self.dots(f, cells(f))
            parts = torch.view_as_real(jv[f.fname]).reshape(K, -1, 2)
            d.index_copy_(1, index[f.fname][0], parts[:, :, 0])
            d.index_copy_(1, index[f.fname][1], parts[:, :, 1])
        _call('emg3d_dev_data_space_filter', M, rank, K, _ptr(pre['q']), _ptr(pre['eigenvalues']), _ptr(pre['s']), _ptr(d),
              _ptr(y), _ptr(table), _ptr(self.fws), fws_len)
        for freq in live:
            f = self.stage(freq)
            re, im = index[f.fname]
            coef = torch.complex(y[:, re], -y[:, im]).reshape(jv[f.fname].shape)       # conj, as for ``jtvec``
            self.combine(f, coef, list(range(K)))
        return grad


def _svqb_rotation(G):
    """The matrix T (K, r) of one SVQB step (Stathopoulos and Wu) from the Gram matrix ``G = Y^T Y`` (K, K) of a block:
    with ``D = diag G``, ``D^-1/2 G D^-1/2 = Z L Z^T`` (``eigh``, fp64) and the r eigenvalues above ``K eps max L``,
    largest first, ``T = D^-1/2 Z L^-1/2`` -- the columns of ``Y T`` are orthonormal. The scaling takes the norms of the
    columns out of the spectrum, the threshold reveals the rank: r < K for a block of dependent columns, 0 for a block
    of zeros. A column whose norm is 0 (or not finite) gets a row of zeros."""
    K = len(G)
    d = np.diag(G)
    with np.errstate(divide='ignore', invalid='ignore'):
        scale = np.where((d > 0) & np.isfinite(d), 1.0 / np.sqrt(d), 0.0)
    lam, Z = np.linalg.eigh(G * scale[:, None] * scale[None, :])
    lam, Z = lam[::-1], Z[:, ::-1]
    r = int(np.sum(lam > K * np.finfo(float).eps * max(lam[0], 0.0))) if lam[0] > 0 else 0
    return np.ascontiguousarray(scale[:, None] * Z[:, :r] / np.sqrt(lam[:r])[None, :])


class _BlockOrth:
    """Makes the columns of a device block orthonormal in place: SVQB on the Gram matrix, applied twice.
    Per application one ``emg3d_dev_block_gram``, the download of (K, K), ``_svqb_rotation`` on the host, the upload of
    T and one ``emg3d_dev_block_rotate`` -- the first from the block into the scratch, the second back. The object owns
    the scratch, one second block of ``kmax`` columns, the workspace of the sums and the two small matrices; every call
    uses them again. ``rotate`` serves other products ``Y T`` of the caller (into the scratch)."""

    def __init__(self, dev, kmax, n):
        need, free = kmax * n * 8, free_hbm(dev)
        if need > free:
            raise MemoryError(f"ReciprocalSensitivity: the second block of {kmax} columns that the orthonormalisation "
                              f"needs takes {need:,} B of HBM, {free:,} B are free.")
        self.n, self.kmax = n, kmax
        self.other = torch.empty((kmax, n), dtype=torch.float64, device=dev)
        self.g, self.t = (torch.empty(kmax * kmax, dtype=torch.float64, device=dev) for _ in range(2))
        self.ws = torch.empty(_lib.lib().emg3d_block_gram_ws_len(n, kmax), dtype=torch.float64, device=dev)

    def gram(self, block):
        """``block`` (K, n) -> its Gram matrix (K, K) on the host."""
        K = len(block)
        _call('emg3d_dev_block_gram', self.n, K, _ptr(block), block.stride(0), _ptr(self.g), _ptr(self.ws))
        return self.g[:K * K].cpu().numpy().reshape(K, K)

    def rotate(self, block, T, out=None):
        """``out`` (default: the scratch) = ``block`` (K, n) times the host matrix T (K, r): (r, n)."""
        K, r = T.shape
        out = self.other[:r] if out is None else out
        self.t[:K * r].copy_(torch.from_numpy(np.ascontiguousarray(T, dtype=np.float64)).view(-1))
        _call('emg3d_dev_block_rotate', self.n, K, r, _ptr(block), block.stride(0), _ptr(self.t), _ptr(out), out.stride(0))
        return out

    def __call__(self, block):
        """``block`` (K, n), K <= kmax, contiguous: (its first ``rank`` rows, now orthonormal and spanning what the K
        rows spanned; rank). The block is overwritten."""
        T = _svqb_rotation(self.gram(block))
        if T.shape[1] == 0:
            return block[:0], 0
        first = self.rotate(block, T)
        T = _svqb_rotation(self.gram(first))
        if T.shape[1] == 0:
            return block[:0], 0
        return self.rotate(first, T, block[:T.shape[1]]), T.shape[1]


class _BlockPCG:
    """The state and the step of the block PCG of ``gauss_newton_solve`` for the K columns of the pass ``ps``, all in
    HBM: ``x`` = 0, the residual ``r`` (the right-hand sides as given: updated in place), ``p``, the table of the
    per-column scalars (lambda, <b,b>, <r,z> new / old, <p,q>, <r,r>, iterations, state), the dampings ``lam``, ``pq``,
    the workspaces of the sums (``ws``) and of the regulariser (``rws``). ``diagonals`` = (diag H, diag R) on the device
    make Jacobi, ``rd_rows`` says that diag R has a row per component (the entry points ``_rd``); with ``blocks`` the
    first of ``diagonals`` holds the packed cell blocks (n (n + 1) / 2, n_cells) instead and makes block-Jacobi (the
    entry points ``_blk``); ``pre``, the dict of ``_data_preconditioner_setup``, makes the data-space preconditioner with
    its blocks ``u`` and ``z`` = M r. The four variants are the entry points and argument tails chosen here; everything
    is queued, nothing is waited for."""

    def __init__(self, ps, lam, r, tol, dmask=None, diagonals=(None, None), rd_rows=False, pre=None, blocks=False):
        L, dev = _lib.lib(), ps.dev
        K, n, ncell = r.shape
        self.ps, self.pre, self.tol, self.r, self.shape = ps, pre, float(tol), r, (ncell, n, K)
        self.x, self.p = torch.zeros_like(r), torch.zeros_like(r)
        host = np.zeros((K, L.emg3d_pcg_table_len(K) // K))
        host[:, 0] = lam
        self.table = torch.from_numpy(host).to(dev)
        self.lam = torch.from_numpy(lam).to(dev)
        self.pq = torch.zeros(K, dtype=torch.float64, device=dev)
        self.ws = torch.empty(L.emg3d_pcg_ws_len(ncell, K), dtype=torch.float64, device=dev)
        self.rws = torch.empty(L.emg3d_model_regulariser_ws_len(*ps.rec.model.grid.shape_cells, K * n, n),
                               dtype=torch.float64, device=dev)
        self.held = diagonals + (dmask,)
        hd, rd, self.mask = (None if t is None else _ptr(t) for t in self.held)
        rd_rows = rd_rows and pre is None
        if blocks:
            sfx, diag = '_blk', (hd, ncell, rd, ncell if rd_rows else 0, self.mask)
        else:
            sfx = '_rd' if rd_rows else ''
            diag = (hd, rd) + ((ncell,) if rd_rows else ()) + (self.mask,)
        self.sums = (_ptr(self.table), _ptr(self.pq), _ptr(self.ws), self.ws.numel())
        self._update = ('emg3d_dev_pcg_update' + sfx, diag + self.sums)
        if pre is None:
            self._direction = ('emg3d_dev_pcg_direction' + sfx, (_ptr(r),) + diag + self.sums[:1])
        else:                                            # x, r as without a preconditioner; z = M r is stored
            self.u, self.z = torch.zeros_like(r), torch.zeros_like(r)
            self.dinv = (_ptr(pre['dinv']), pre['dinv_stride'])
            self._direction = ('emg3d_dev_pcg_direction_z', (_ptr(self.z),) + self.sums[:1])

    def update(self, first, q=None):
        name, tail = self._update
        _call(name, *self.shape, first, _ptr(self.x), _ptr(self.r), _ptr(self.p), None if q is None else _ptr(q), *tail)

    def scale(self, first):
        _call('emg3d_dev_pcg_scale', *self.shape, first, _ptr(self.u), _ptr(self.r), *self.dinv, *self.sums[:2])

    def finish(self, first, g):
        _call('emg3d_dev_pcg_finish', *self.shape, first, _ptr(self.z), _ptr(self.u), _ptr(g), _ptr(self.r), *self.dinv,
              self.mask, *self.sums)

    def precondition(self, first):
        """``z = M r`` for the running columns: ``scale`` (u), one ``precondition`` pass over the kept fields (g = J^T
        y), ``finish`` (z, and the partial sums of <r, z> and <r, r>, which overwrite those of ``update``)."""
        self.scale(first)
        self.finish(first, self.ps.rec._gradient_block(self.ps.precondition(self.u, self.pre, self.table)))
        return self.z

    def scalar(self, first):
        ncell, n, K = self.shape
        _call('emg3d_dev_pcg_scalar', ncell, K, first, self.tol, *self.sums)

    def direction(self, first):
        name, tail = self._direction
        _call(name, *self.shape, first, _ptr(self.p), *tail)

    def step(self, first, q=None):
        """One step with ``q = (H + lambda R) p`` (the set-up, ``first`` = 1: without): the update kernel, the
        preconditioner application if there is one, the scalar kernel, the direction kernel."""
        self.update(first, q)
        if self.pre is not None:
            self.precondition(first)
        self.scalar(first)
        self.direction(first)
