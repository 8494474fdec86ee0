"""Data misfit and adjoint-state gradient.

The reference obtains both from ``Simulation`` (emg3d/simulations.py:943-1094 ``gradient``,
:1097-1190 ``misfit``, :1193-1268 ``_bcompute`` / ``_get_rfield``) whose bookkeeping lives in
xarray datasets and whose solves run in a process pool. Here the same computation is a plain
function over (source, frequency) pairs, sharded over the ranks of the process group like the
forward solves of ``parallel.compute``:

    per pair, on its GPU
      1. forward solve                      -> efield stays in HBM
      2. responses at the receivers         (linear interpolation on the device, as the exact
                                             adjoint requires, simulations.py:975-983)
      3. residual = synthetic - observed;   misfit += sum w |residual|^2 / 2
      4. residual source field              = sum over receivers of a point dipole at the receiver
                                              with strength conj(residual w / (-s mu0))
      5. back-propagated solve, same hierarchy (levels, line factors, graphs)  -> bfield in HBM
      6. gradient += cells(real(bfield s mu0 efield))      (emg3d_dev_gradient_accumulate)
    once
      7. all-reduce of the cell gradient and of the misfit over the ranks (RCCL)
      8. anisotropy bookkeeping and the derivative chain of the property mapping (host, one pass)

Computational grids that differ from the model grid (``grids=``): the model goes to the pair's grid
by volume averaging (``Model.interpolate_to_grid``), the cell gradient comes back through the
adjoint of the linear averaging (``models._VolumeAverage.adjoint_add``; the reference takes that
operator from discretize, ``maps._interp_volume_average_adj``, emg3d/maps.py:722-750).

Magnetic point receivers (``magnetic=``): responses = ``get_magnetic_field`` interpolated linearly to the
point, adjoint source = the transpose of exactly that map (``fields.get_magnetic_point_source_field``;
the reference builds its ``_point_vector_magnetic`` from discretize's operators, emg3d/fields.py:749-789).

Sensitivity products (``Sensitivity``, ``jvec``, ``jtvec``; reference ``Simulation.jvec`` / ``jtvec``,
emg3d/simulations.py:1271-1434): a Gauss-Newton step multiplies the sensitivity matrix J (derivative of the
complex responses with respect to the model properties) and its adjoint with vectors many times at ONE model.
``Sensitivity`` is that linearisation point: it computes the forward fields once and keeps them per pair (in
HBM, in pinned host memory, or not at all), and then

    jvec(v)  = P A^-1 G v       G v: cells -> edges, times the forward field, times -s mu0
                                (emg3d_dev_sensitivity_source, written into the hierarchy's source vector);
                                one solve per pair at ``tol_gradient``; P: the receivers' linear interpolation
    jtvec(y) = G^H A^-H P^H y   steps 4-8 above with ``residual w`` replaced by ``y`` and the KEPT forward
                                field in step 6 (emg3d_dev_gradient_accumulate is the transpose of G)

Convention: ``jtvec`` returns the real array with ``sum(v * jtvec(y)) == Re sum_i conj(y_i) jvec(v)_i`` for
every real ``v`` -- which makes ``misfit_and_gradient == jtvec(residual * weights)`` the gradient of
``sum w |r|^2 / 2``.

``ReciprocalSensitivity`` keeps one more field per (receiver, frequency), the solution for a unit datum at that
receiver; A being complex symmetric, both products are then reductions over the kept fields and solve nothing
(DESIGN.md 4.12).

Limits as in the reference: no epsilon_r / mu_r.
"""
import numpy as np

from emg3d_amd import fields, models
from emg3d_amd.fields import Field

__all__ = ['misfit_and_gradient', 'residual_source_field', 'Sensitivity', 'ReciprocalSensitivity', 'jvec', 'jtvec',
           'expand_vector']

_DCHAIN = {          # d sigma / d property, applied to the gradient w.r.t. conductivity (emg3d/maps.py:120-330)
    'Conductivity': lambda g, p: g,
    'Resistivity': lambda g, p: g * -(1.0 / p) ** 2,
    'LgConductivity': lambda g, p: g * (10.0 ** p) * np.log(10.0),
    'LgResistivity': lambda g, p: g * -(10.0 ** -p) * np.log(10.0),
    'LnConductivity': lambda g, p: g * np.exp(p),
    'LnResistivity': lambda g, p: g * -np.exp(-p),
}


def residual_source_field(grid, frequency, receivers, residual, weight, magnetic=None):
    """Source field of the back-propagation (``Simulation._get_rfield``, simulations.py:1235-1268):
    every receiver with data acts as a point dipole of strength ``conj(residual weight / (-s mu0))``
    -- an electric one (``TxElectricPoint``: the adjoint of the tri-linear receiver interpolation) or,
    for the receivers flagged in ``magnetic``, a magnetic one (``TxMagneticPoint``).
    ``receivers``: sequence of (x, y, z, azimuth, elevation); ``residual`` / ``weight``: one value per
    receiver (NaN residual: no data)."""
    rfield = Field(grid, frequency=frequency)
    strength = np.conj(np.asarray(residual) * np.asarray(weight) / -rfield.smu0)
    magnetic = np.zeros(len(strength), dtype=bool) if magnetic is None else np.asarray(magnetic, dtype=bool)
    index, value = [], []
    for rec, res, st, mag in zip(receivers, np.asarray(residual), strength, magnetic):
        if np.isnan(res):
            continue
        make = fields.get_magnetic_point_source_field if mag else fields.get_point_source_field
        part = make(grid, tuple(rec), frequency, strength=st)
        index.append(part._sparse[0])
        value.append(part._sparse[1])
    if index:
        index, value = np.concatenate(index), np.concatenate(value)
        np.add.at(rfield._field, index, value)
        nz = np.unique(index)
        rfield._sparse = (nz, rfield._field[nz].copy())
    else:
        rfield._sparse = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=rfield._field.dtype))
    return rfield


def _receiver_tuple(receivers):
    r = np.asarray(receivers, dtype=float)
    return tuple(r[:, k] for k in range(5))


def misfit_and_gradient(model, sources, frequencies, receivers, observed, weights=None, solver_opts=None,
                        tol_gradient=1e-5, costs=None, grids=None, interpolate_opts=None, magnetic=None):
    """Misfit ``sum w |synthetic - observed|^2 / 2`` and its adjoint-state gradient with respect to
    the model properties (shape (nx, ny, nz) for isotropic models, (2, ...) HTI / VTI, (3, ...)
    tri-axial, as ``Simulation.gradient``).

    sources: dict name -> source coordinates; frequencies: dict name -> Hz; receivers: sequence of
    (x, y, z, azimuth, elevation) point receivers -- electric ones, or magnetic ones where the boolean
    sequence ``magnetic`` says so (responses in A/m: ``get_magnetic_field`` at the point); observed / weights: dict
    (source name, frequency name) -> one value per receiver (NaN: no data; weights default 1).
    grids: the computational grid of the pairs, if it is not the model's: one TensorMesh for all, or
    a dict (source name, frequency name) -> TensorMesh (pairs that are missing use the model grid);
    interpolate_opts: passed to ``Model.interpolate_to_grid`` (default: averaging on a log10 scale, as
    in the reference -- the way back is the adjoint of the LINEAR averaging either way, exact for
    ``{'log': False}`` with a conductivity model).
    With an initialised process group the pairs are sharded over the ranks and both results are
    all-reduced: every rank returns the complete misfit and gradient."""
    from emg3d_amd import _lib
    _lib.require_gpu()
    lin = Sensitivity(model, sources, frequencies, receivers, solver_opts=solver_opts, tol_gradient=tol_gradient,
                      costs=costs, grids=grids, interpolate_opts=interpolate_opts, magnetic=magnetic, keep=False)
    lin._order = list(lin._mine)          # pair by pair in the order of the shard, as ever
    try:
        misfit, grad = lin.misfit_and_gradient(observed, weights)
        return misfit, grad, lin.info
    finally:
        lin.release()


def _check_model(model):
    for name, prop in (('el. permittivity', model.epsilon_r), ('magn. permeability', model.mu_r)):
        if prop is not None and not np.allclose(prop, 1.0):
            raise NotImplementedError(f"Gradient not implemented for {name}.")


_NCOMP = {'isotropic': 1, 'HTI': 2, 'VTI': 2, 'triaxial': 3}
_EXPAND = {'isotropic': (0, 0, 0), 'HTI': (0, 1, 0), 'VTI': (0, 0, 1), 'triaxial': (0, 1, 2)}


_PROPS = {'isotropic': ('property_x',), 'HTI': ('property_x', 'property_y'), 'VTI': ('property_x', 'property_z'),
          'triaxial': ('property_x', 'property_y', 'property_z')}


def _check_vector(model, vector):
    """The model-shaped ``vector`` of ``jvec`` as (n, nx, ny, nz) floats -- n = 1 (isotropic), 2 (HTI: x, y; VTI:
    x, z) or 3; raises unless it is real and shaped like the model's properties."""
    n, shape = _NCOMP[model.case], tuple(model.grid.shape_cells)
    v = np.asarray(vector)
    allowed = [(n,) + shape] + ([shape] if n == 1 else [])
    if v.shape not in allowed or np.iscomplexobj(v):
        raise ValueError(f"`vector` must be real with shape {' or '.join(str(a) for a in allowed[::-1])} "
                         f"for a model of case '{model.case}'. Provided: {v.dtype} {v.shape}.")
    return np.asarray(v, dtype=np.float64).reshape((n,) + shape)


def _vector_components(model, vector):
    """The model-shaped ``vector`` of ``jvec`` as (n, nx, ny, nz) floats after the derivative chain of the
    mapping, ``vector_k * d sigma / d property_k`` -- n = 1 (isotropic), 2 (HTI: x, y; VTI: x, z) or 3."""
    v = _check_vector(model, vector)
    chain = _DCHAIN[model.mapping]
    return np.stack([chain(v[k], np.asarray(getattr(model, name), dtype=float))
                     for k, name in enumerate(_PROPS[model.case])])


def expand_vector(model, vector):
    """What ``jvec`` hands to ``G``: ``vector`` after the derivative chain of the mapping, expanded to the
    three conductivity components (3, nx, ny, nz) -- isotropic (v, v, v), HTI (v0, v1, v0), VTI (v0, v0, v1),
    tri-axial as given (emg3d/simulations.py:1314-1349)."""
    comps = _vector_components(model, vector)
    return comps[list(_EXPAND[model.case])]


def _finish_gradient(model, g3):
    """Anisotropy bookkeeping + derivative chain of the mapping (simulations.py:1070-1090) for the gradient
    with respect to the three conductivity components, (3, nx, ny, nz)."""
    chain = _DCHAIN[model.mapping]
    keep = [0]
    if model.case in ('HTI', 'triaxial'):
        g3[1] = chain(g3[1], model.property_y)
        keep.append(1)
    else:
        g3[0] += g3[1]
    if model.case in ('VTI', 'triaxial'):
        g3[2] = chain(g3[2], model.property_z)
        keep.append(2)
    else:
        g3[0] += g3[2]
    g3[0] = chain(g3[0], model.property_x)
    return np.asfortranarray(g3[keep].squeeze())


class Sensitivity:
    """One linearisation point: model, survey geometry, and the forward fields of its pairs.

    Parameters as ``misfit_and_gradient`` (sources, frequencies, receivers, solver_opts, tol_gradient, costs,
    grids, interpolate_opts, magnetic), plus

    keep: where the forward field of a pair lives between calls -- ``'device'`` (an HBM tensor,
        ``n_edges x 16 B`` per pair of this rank: 0.8 GB at 256^3), ``'host'`` (a pinned host buffer,
        uploaded when used) or ``False`` (recomputed by every call: what ``misfit_and_gradient`` costs).
    batch: > 1: up to that many of the rank's pairs that share frequency and computational grid are solved
        TOGETHER by ``solver.solve_batch`` in ``jvec`` and ``jtvec`` (multigrid: bit-identical to pair by
        pair; BiCGSTAB: each source its own iteration, equal to the tolerance). Pairs with magnetic
        receivers, cgs and gcrotmk stay pair by pair.

    With an initialised process group the pairs are sharded over the ranks at construction (kept fields stay
    on the rank that owns the pair); ``jvec`` and ``synthetic`` are complete on every rank, ``jtvec`` is
    all-reduced. ``n_solves`` counts the solves this rank ran: ``{'forward', 'jvec', 'jtvec'}``.
    """

    def __init__(self, model, sources, frequencies, receivers, solver_opts=None, tol_gradient=1e-5, costs=None,
                 grids=None, interpolate_opts=None, magnetic=None, keep='device', batch=1):
        from emg3d_amd import parallel
        _check_model(model)
        if keep not in ('device', 'host', False, None):
            raise ValueError(f"`keep` must be 'device', 'host' or False. Provided: {keep!r}.")
        self.model, self.sources, self.frequencies = model, dict(sources), dict(frequencies)
        self.receivers = np.asarray(receivers, dtype=float)
        self.opts = dict(solver_opts or {})
        self.opts.setdefault('sslsolver', True)
        self.tol_gradient = tol_gradient
        self.grids, self.interpolate_opts = grids, interpolate_opts
        self.keep = keep or False
        self.batch = max(1, int(batch))
        self._rec = _receiver_tuple(self.receivers)
        nrec = len(self._rec[0])
        self._mag = np.zeros(nrec, dtype=bool) if magnetic is None else np.asarray(magnetic, dtype=bool)
        self.pairs = parallel.srcfreq_pairs(self.sources, self.frequencies)
        self.rank, self.world = parallel.rank_and_world()
        self._mine = parallel.shard(len(self.pairs), self.rank, self.world, costs)
        forder = {f: n for n, f in enumerate(self.frequencies)}
        # pairs of one frequency next to each other: every hierarchy is built once per call
        self._order = sorted(self._mine, key=lambda i: (forder[self.pairs[i][1]], i))
        self.n_solves = {'forward': 0, 'jvec': 0, 'jtvec': 0}
        self.info = {}
        self._reset()

    def _reset(self):
        self._kept = {}              # pair index -> forward field (device tensor / pinned host tensor)
        self._synthetic = {}         # pair index -> responses of the forward field (this rank's pairs)
        self._all_synthetic = None
        self._hier = {}              # (s, grid key, batch) -> Hierarchy; one (frequency, grid) at a time
        self._on_grid = {}
        self._have_forward = False

    def __repr__(self):
        return (f"Sensitivity: {len(self.pairs)} pairs ({len(self._mine)} on rank {self.rank} of {self.world}); "
                f"keep={self.keep!r}, batch={self.batch}; kept forward fields: {len(self._kept)} x "
                f"{self.kept_bytes // max(len(self._kept), 1):,} B = {self.kept_bytes:,} B "
                f"({ {'device': 'HBM', 'host': 'pinned host memory'}.get(self.keep, 'nothing kept') })")

    @property
    def kept_bytes(self):
        """Bytes held by the kept forward fields of this rank (n_pairs_on_rank x n_edges x 16 B, complex)."""
        return int(sum(t.numel() * t.element_size() for t in self._kept.values()))

    def release(self):
        """Drop the kept fields, the hierarchies and the per-grid tables."""
        self._reset()

    # ----------------------------------------------------------------------------- pieces ---
    def _device(self):
        import torch
        from emg3d_amd import _lib
        _lib.require_gpu()
        return torch.device('cuda', torch.cuda.current_device())

    def _grid_of(self, pair):
        """The computational grid of a pair; the model's own grid object where ``grids`` gives none or an equal one."""
        g = self.grids.get(pair) if isinstance(self.grids, dict) else self.grids
        return self.model.grid if g is None or g == self.model.grid else g

    def _require_model_grid(self, what, why):
        """Raises for the product ``what`` unless every pair is computed on the model grid."""
        for pair in self.pairs:
            if self._grid_of(pair) is not self.model.grid:
                raise NotImplementedError(f"{what}: the computational grid of {pair!r} (`grids`) is not the model grid; "
                                          f"there every row of the sensitivity needs its own adjoint volume average {why}.")

    def _computational(self, pair):
        """(grid key, grid, model on it, cell volumes in HBM, averaging plan or None) of a pair."""
        import torch
        mgrid = self.model.grid
        g = self._grid_of(pair)
        key = id(g) if g is not mgrid else 0
        if key not in self._on_grid:
            vol = torch.from_numpy(np.ascontiguousarray(g.cell_volumes, dtype=np.float64)).to(self._device())
            plan = None if g is mgrid else models._VolumeAverage(mgrid, g)
            self._on_grid[key] = (g, self.model.interpolate_to_grid(g, **(self.interpolate_opts or {})), vol, plan)
        return (key,) + self._on_grid[key]

    def _hierarchy(self, gkey, gmodel, meta, batch=1):
        from emg3d_amd import solver
        hkey = (complex(meta.sval), gkey, batch)
        hier = self._hier.get(hkey)
        if hier is None:
            if any(k[:2] != hkey[:2] for k in self._hier):
                self._hier.clear()                    # one (frequency, grid) at a time in HBM
            hier = self._hier[hkey] = solver.Hierarchy(models.VolumeModel(gmodel, meta), batch=batch)
        return hier

    def _solve_forward(self, i):
        """Forward solve of pair i: (field in HBM -- a copy, the hierarchy's own buffer is reused --, responses)."""
        import torch
        from emg3d_amd import solver
        from emg3d_amd._device import copy
        sname, fname = self.pairs[i]
        freq = self.frequencies[fname]
        gkey, grid, gmodel, vol, plan = self._computational((sname, fname))
        sfield = fields.get_source_field(grid, self.sources[sname], freq)
        hier = self._hierarchy(gkey, gmodel, sfield)
        top = hier.top
        _, finfo = solver.solve(gmodel, sfield, return_info=True, always_return=True, hierarchy=hier, _download=False,
                                _sparse_source=True, **self.opts)
        self.n_solves['forward'] += 1
        e_fwd = torch.empty_like(top.e)
        copy(e_fwd, top.e)
        synthetic = fields.get_responses(Field(grid, frequency=freq), e_fwd, self._rec, 'linear', magnetic=self._mag)
        self.info.setdefault((sname, fname), {}).update(forward=finfo, backward=None, synthetic=synthetic)
        return e_fwd, synthetic

    def _forward_field(self, i):
        """Forward field of pair i in HBM and its responses: the kept one, or a new solve (``keep=False``)."""
        import torch
        if i in self._kept:
            e = self._kept[i]
            if self.keep == 'host':
                e = e.to(self._device(), non_blocking=False)
            return e, self._synthetic[i]
        e, synthetic = self._solve_forward(i)
        self._synthetic[i] = synthetic
        if self.keep == 'device':
            self._kept[i] = e
        elif self.keep == 'host':
            pinned = torch.empty(e.shape, dtype=e.dtype, pin_memory=True)
            pinned.copy_(e)
            self._kept[i] = pinned
        return e, synthetic

    def forward(self):
        """Forward solves of this rank's pairs at ``solver_opts['tol']`` (once; later calls return at once, and
        with ``keep=False`` only the responses are kept)."""
        if not self._have_forward:
            for i in self._order:
                self._forward_field(i)
            self._have_forward = True
        return self

    @property
    def synthetic(self):
        """Forward responses: dict (src, freq) -> complex array (n_receivers), complete on every rank."""
        if self._all_synthetic is None:
            self.forward()
            self._all_synthetic = self._gather({self.pairs[i]: self._synthetic[i] for i in self._mine})
        return self._all_synthetic

    def _gather(self, local):
        """The union of the ranks' small dicts, on every rank, in the order of ``pairs``."""
        if self.world > 1:
            from emg3d_amd import parallel
            parts = [None] * self.world
            parallel._dist().all_gather_object(parts, local)
            local = {k: v for part in parts for k, v in part.items()}
        return {p: local[p] for p in self.pairs if p in local}

    def _may_batch(self):
        """Whether solves may go through ``solve_batch`` (the rules of ``batch`` in the class docstring)."""
        return (self.batch > 1 and not self._mag.any() and
                self.opts.get('sslsolver', True) in (True, False, None, 'bicgstab') and
                self.opts.get('cycle', 'F') is not None)

    def _chunks(self):
        """This rank's pairs in solve order, grouped for ``solve_batch``: lists of up to ``batch`` pair indices
        that share frequency and computational grid (lists of one: pair by pair)."""
        batched = self._may_batch()
        chunks = []
        for i in self._order:
            key = (self.pairs[i][1], self._computational(self.pairs[i])[0])
            if batched and chunks and chunks[-1][0] == key and len(chunks[-1][1]) < self.batch:
                chunks[-1][1].append(i)
            else:
                chunks.append((key, [i]))
        return [c for _, c in chunks]

    # ------------------------------------------------------------------------------- jvec ---
    @staticmethod
    def _cells_on_device(comps, dev):
        """Cell arrays (nx, ny, nz) as flat device tensors, x fastest, as the kernels index them (the transposition
        of a C-ordered array runs on the device)."""
        import torch
        return [torch.from_numpy(np.ascontiguousarray(c)).to(dev).permute(2, 1, 0).contiguous().reshape(-1)
                for c in comps]

    def jvec(self, vector):
        """Sensitivity times a model-shaped real ``vector`` -- shape (nx, ny, nz) or (1, ...) isotropic,
        (2, ...) HTI / VTI, (3, ...) tri-axial, as ``Simulation.jvec``: dict (src, freq) -> complex array
        (n_receivers), complete on every rank. One solve per pair at ``tol_gradient``; a zero vector gives
        zeros without a solve."""
        import torch
        from emg3d_amd import _lib, solver
        from emg3d_amd._device import _ptr, _stream
        comps = _vector_components(self.model, vector)          # raises on a wrong shape, before any GPU work
        dev = self._device()
        expand = _EXPAND[self.model.case]
        on_model = self._cells_on_device(comps, dev)
        regridded = {0: on_model}
        opts = {**self.opts, 'tol': self.tol_gradient}
        out = {}
        for chunk in self._chunks():
            nb = len(chunk)
            sname, fname = self.pairs[chunk[0]]
            freq = self.frequencies[fname]
            gkey, grid, gmodel, vol, plan = self._computational((sname, fname))
            if gkey not in regridded:            # linear volume average: the map whose adjoint is jtvec's way back
                regridded[gkey] = [plan.on_device(c, log=False) for c in on_model]
            vx, vy, vz = (regridded[gkey][k] for k in expand)
            meta = Field(grid, frequency=freq)
            smu0 = complex(meta.smu0)
            nx, ny, nz = grid.shape_cells
            n, o1, o2 = grid.n_edges, grid.n_edges_x, grid.n_edges_x + grid.n_edges_y
            forward = [self._forward_field(i)[0] for i in chunk]      # (before the batch hierarchy replaces another)
            hier = self._hierarchy(gkey, gmodel, meta, nb)
            top = hier.top
            for b, e in enumerate(forward):
                _lib.check(_lib.lib().emg3d_dev_sensitivity_source(
                    nx, ny, nz, int(top.is_complex), _ptr(e), _ptr(e, o1), _ptr(e, o2), smu0.real, smu0.imag,
                    _ptr(vol), _ptr(vx), _ptr(vy), _ptr(vz), _ptr(top.s, b * n), _ptr(top.s, b * n + o1),
                    _ptr(top.s, b * n + o2), _stream()), 'emg3d_dev_sensitivity_source')
            del forward
            if nb == 1:
                _, info = solver.solve(gmodel, meta, return_info=True, always_return=True, hierarchy=hier,
                                       _download=False, _device_source=True, **opts)
                infos = [info]
                resp = [fields.get_responses(meta, top.e, self._rec, 'linear', magnetic=self._mag)]
            else:
                res = solver.solve_batch(gmodel, [Field(grid, frequency=freq) for _ in chunk], receivers=self._rec,
                                         receiver_method='linear', keep_fields=False, hierarchy=hier,
                                         _device_sources=True, **opts)
                infos = [info for _, info in res]
                resp = [np.asarray(info['responses']) for info in infos]
            for i, info, r in zip(chunk, infos, resp):
                self.n_solves['jvec'] += int(not np.isnan(info['ref_error']))     # (NaN: zero source, nothing solved)
                self.info.setdefault(self.pairs[i], {})['jvec'] = info
                out[self.pairs[i]] = np.asarray(r)
        return self._gather(out)

    # ------------------------------------------------------------------------------ jtvec ---
    def _check_data(self, vector):
        """Raises unless every entry of the data-shaped ``vector`` has one value per receiver; their number."""
        nrec = len(self._rec[0])
        for pair, y in vector.items():
            if np.shape(y) != (nrec,):
                raise ValueError(f"`vector[{pair!r}]` must have shape ({nrec},): one value per receiver. "
                                 f"Provided: {np.shape(y)}.")
        return nrec

    def jtvec(self, vector):
        """Adjoint of the sensitivity times a data-shaped ``vector`` -- dict (src, freq) -> complex array
        (n_receivers), NaN or a missing pair: no datum --: real array shaped like the gradient of
        ``misfit_and_gradient``, with ``sum(v * jtvec(y)) == Re sum conj(y) * jvec(v)``. One solve per pair at
        ``tol_gradient`` against the kept forward field; all-reduced over the ranks."""
        nrec = self._check_data(vector)

        def data(pair, synthetic):
            y = vector.get(pair)
            return (None, None) if y is None else (np.asarray(y), np.ones(nrec))      # (real in the Laplace domain)
        return self._back_propagate(data)[1]

    def misfit_and_gradient(self, observed, weights=None):
        """Misfit ``sum w |synthetic - observed|^2 / 2`` and its gradient ``jtvec((synthetic - observed) w)``,
        from the kept forward fields."""
        def data(pair, synthetic):
            obs = np.asarray(observed[pair])
            w = np.ones(obs.shape) if weights is None else np.asarray(weights[pair], dtype=float)
            return synthetic - obs, w
        return self._back_propagate(data, with_misfit=True)

    def _solve_residual_sources(self, gkey, gmodel, meta, rfields, opts):
        """The solutions for the residual source fields ``rfields`` of one frequency and grid, one ``solve`` or one
        ``solve_batch``: a list of (field in HBM -- ``None``: the solve failed --, solver info). The field of a single
        source is the hierarchy's own ``top.e``: the next solve overwrites it."""
        from emg3d_amd import solver
        hier = self._hierarchy(gkey, gmodel, meta, len(rfields))
        if len(rfields) == 1:
            _, info = solver.solve(gmodel, rfields[0], return_info=True, always_return=True, hierarchy=hier,
                                   _download=False, _sparse_source=True, **opts)
            return [(hier.top.e, info)]
        for rf in rfields:
            rf._trust_sparse = True
        res = solver.solve_batch(gmodel, rfields, keep_fields=False, hierarchy=hier, _device_fields=True, **opts)
        return [(info.pop('_device_field', None), info) for _, info in res]

    @staticmethod
    def _on_model_grid(plan, grid, target, launch):
        """``launch(gtarget, nc)`` adds a cell gradient to the three rows of ``nc`` cells at ``gtarget``: into ``target``,
        (3, n_cells) on the model grid, at once, or (``plan``: the averaging plan of another computational ``grid``) on
        that grid first and from there through the adjoint of the linear volume average, target += P^T g."""
        import torch
        if plan is None:
            return launch(target.view(-1), target.shape[1])
        nc = grid.n_cells
        gtarget = torch.zeros(3 * nc, dtype=torch.float64, device=target.device)
        launch(gtarget, nc)
        for k in range(3):
            plan.adjoint_add(gtarget[k * nc:(k + 1) * nc], target[k])

    def _back_propagate(self, data, with_misfit=False):
        """``data(pair, synthetic) -> (residual, weight)`` per receiver: steps 3-8 of the module docstring for
        this rank's pairs. Returns (misfit of the residuals if asked for, gradient)."""
        import torch
        from emg3d_amd import _lib, parallel
        from emg3d_amd._device import _ptr, _stream
        dev = self._device()
        grad = torch.zeros((3, self.model.grid.n_cells), dtype=torch.float64, device=dev)
        misfit = 0.0
        opts = {**self.opts, 'tol': self.tol_gradient}
        for chunk in self._chunks():
            sname, fname = self.pairs[chunk[0]]
            freq = self.frequencies[fname]
            gkey, grid, gmodel, vol, plan = self._computational((sname, fname))
            nx, ny, nz = grid.shape_cells
            forward, rfields = [], []
            for i in chunk:
                pair = self.pairs[i]
                e_fwd, synthetic = self._forward_field(i)
                residual, w = data(pair, synthetic)
                rfield = None
                if residual is not None:
                    have = ~np.isnan(residual)
                    if with_misfit:
                        misfit += float(np.sum(w[have] * (residual[have].conj() * residual[have])).real) / 2
                    # no data (or a perfect fit) for this pair: no residual source, nothing back-propagated,
                    # no contribution (the reference drops such pairs, emg3d/simulations.py:1120-1190)
                    if np.any(have & (residual != 0)):
                        rfield = residual_source_field(grid, freq, self.receivers, residual, w, self._mag)
                forward.append(e_fwd)
                rfields.append(rfield)
            live = [b for b, rf in enumerate(rfields) if rf is not None]
            if not live:
                continue
            meta = Field(grid, frequency=freq)
            back = self._solve_residual_sources(gkey, gmodel, meta, [rfields[b] for b in live], opts)
            smu0 = complex(meta.smu0)
            o1, o2 = grid.n_edges_x, grid.n_edges_x + grid.n_edges_y
            for b, (bfield, binfo) in zip(live, back):
                self.n_solves['jtvec'] += 1
                self.info.setdefault(self.pairs[chunk[b]], {})['backward'] = binfo
                if bfield is None:                         # the solve failed: zero field, no contribution
                    continue
                e_fwd = forward[b]

                def accumulate(gtarget, nc):
                    _lib.check(_lib.lib().emg3d_dev_gradient_accumulate(
                        nx, ny, nz, int(bfield.is_complex()), _ptr(e_fwd), _ptr(e_fwd, o1), _ptr(e_fwd, o2),
                        _ptr(bfield), _ptr(bfield, o1), _ptr(bfield, o2), smu0.real, smu0.imag, _ptr(vol),
                        _ptr(gtarget), _ptr(gtarget, nc), _ptr(gtarget, 2 * nc), _stream()), 'emg3d_dev_gradient_accumulate')
                self._on_model_grid(plan, grid, grad, accumulate)
            del forward, back
        # the one collective of the path: sum over the ranks
        tm = torch.tensor([misfit], dtype=torch.float64, device=dev)
        if self.world > 1:
            dist = parallel._dist()
            cdev = dev if dist.get_backend() == 'nccl' else torch.device('cpu')
            g, m = grad.to(cdev), tm.to(cdev)
            dist.all_reduce(g)
            dist.all_reduce(m)
            grad, tm = g, m
        misfit = float(tm.cpu()[0])
        return misfit, self._gradient_on_host(grad)

    def _gradient_on_host(self, grad):
        """The cell gradient with respect to the three conductivity components (device, 3 x n_cells, x fastest) as
        the model-shaped array of the model's own properties (step 8 of the module docstring)."""
        g3 = np.stack([row.cpu().numpy().reshape(self.model.grid.shape_cells, order='F') for row in grad])
        return _finish_gradient(self.model, g3)


class ReciprocalSensitivity(Sensitivity):
    """``Sensitivity`` whose ``jvec`` and ``jtvec`` solve nothing: next to the forward field of every (source,
    frequency) it keeps one field per (receiver, frequency),

        x_r = A^-1 residual_source_field(unit datum at receiver r alone)          (at ``tol_gradient``).

    The system matrix is complex symmetric (``jtvec`` back-propagates with A, not its adjoint) and the receiver
    operator does not depend on the source, so ``P_r A^-1 g = (A^-1 p_r)^T g`` and, per frequency,

        jvec(v)[s, r] = conj(-s mu0) sum_k w_k e_s[k] x_r[k]         w = cells_to_edges(volumes * v), real
        jtvec(y)      = cells(real(s mu0 t)),    t[k] = sum_s e_s[k] sum_r conj(y[s, r]) x_r[k]

    -- reductions over the kept fields, bound by HBM (``emg3d_dev_edge_weights`` + ``emg3d_dev_sensitivity_dots_block``;
    ``emg3d_dev_sensitivity_combine_block`` + ``emg3d_dev_edges_to_cells``; one column runs the single-vector kernels
    ``k_sensitivity_dots`` / ``k_sensitivity_combine``): no solve, no hierarchy and no receiver
    interpolation in a Gauss-Newton inner iteration. The price: ``n_receivers`` more solves per frequency in
    ``forward()`` (batched by ``solve_batch`` under the rules of ``Sensitivity``'s ``batch``) and their fields.

    Parameters as ``Sensitivity``, except: ``keep`` is ``'device'`` (two HBM stacks per frequency, [n_sources x
    n_edges] and [n_receivers x n_edges]) or ``'host'`` (pinned stacks; a frequency's two stacks are uploaded into
    one reused staging pair when that frequency is processed) -- ``False`` is refused; all pairs of a frequency must
    share ONE computational grid (with a grid per source the receiver fields are not shared); one process only.
    ``n_solves``: ``{'forward', 'receiver', 'jvec', 'jtvec'}``, the last two stay 0. The solver infos of the receiver
    solves: ``info[('receiver', r, frequency name)]``; ``setup_seconds``: wall time ``forward()`` spent in the source
    and in the receiver solves.

    From the same kept fields, again without a solve: ``hessian_diagonal``, the diagonal of the Gauss-Newton Hessian
    ``Re(J^H W J)`` in one pass (``emg3d_dev_hessian_diagonal``), and ``hessian_vec``, the product it
    preconditions; and ``data_gram``, the data-space normal matrix ``J^ diag(m) J^T`` of Occam and data-space
    Gauss-Newton schemes (``emg3d_dev_data_gram``, DESIGN.md 4.14: the rows of ``J^`` are generated in LDS and consumed
    there, never written), with ``stack_data`` / ``unstack_data`` between data dictionaries and its real vectors.

    Many products at this one linearisation point (randomised SVD, trace estimates, block Krylov methods, probing):
    ``jvec_block``, ``jtvec_block`` and ``hessian_vec_block`` take K vectors and read the kept fields once per group of
    ``columns_per_pass`` columns (``emg3d_dev_sensitivity_dots_block`` / ``_combine_block``); a block of
    model vectors may live on the device -- float64 (K, n, n_cells), cells x fastest, ``to_device`` / ``from_device`` --,
    and ``hessian_vec_block`` then takes and returns one without anything crossing the host.

    Their consumer, the inner linear solve of a Gauss-Newton step: ``gauss_newton_solve`` solves ``(Re(J^H W J) + lambda_k
    R) x_k = b_k`` for K dampings at once by preconditioned CG on the device -- the K columns share every
    ``hessian_vec_block`` pass, the rest of an iteration is three fused kernels, the per-column scalars stay in a device
    table (``emg3d_dev_model_regulariser``, ``emg3d_dev_pcg_update`` / ``_scalar`` / ``_direction``);
    ``regulariser_vec_block`` applies the smallness-plus-roughness operator ``R`` on its own. Beside Jacobi it has a
    data-space preconditioner, ``precondition='data'``: the Woodbury inverse of ``lambda_k diag R + J^T W J`` from one
    ``data_gram`` and one eigen-decomposition per call, applied by one more pass over the kept fields.
    For models with several properties per cell (VTI, HTI, tri-axial) ``hessian_cell_blocks`` gives the n x n blocks of
    ``Re(J^H W J)`` that couple the properties of one cell, in the one pass of ``hessian_diagonal``
    (``emg3d_dev_hessian_cell_blocks``), and ``precondition='block'`` inverts them per cell inside the PCG kernels
    (block-Jacobi, ``emg3d_dev_pcg_update_blk`` / ``_direction_blk``).
    The outer inversion loop (line search, observed data, choice of the damping) is the user's.

    The other consumer, after the step: ``sensitivity_svd``, a randomised truncated SVD ``W^1/2 J^ ~ U diag(s) V^T`` of the
    weighted sensitivity from ``2 + 2 power_iterations`` half passes of the block products, whatever the number of data
    is and on any computational grid -- a step from a truncated pseudo-inverse, the model resolution ``V V^T``, posterior
    variances, the effective rank of a survey. Its two primitives serve any subspace method on device blocks:
    ``orthonormalise_block`` makes the columns of a block orthonormal and reveals its rank (Gram-based SVQB applied
    twice: ``emg3d_dev_block_gram``, ``eigh`` of the small matrix on the host, ``emg3d_dev_block_rotate``; DESIGN.md
    4.21).

    field_dtype: ``'double'`` (default) keeps the fields as they are solved, ``n_edges x 16 B`` each. ``'single'``
        keeps them as complex64 (Laplace domain: float32): half the bytes in HBM or pinned memory, over PCIe with
        ``keep='host'``, and through the two HBM-bound products. Only the STORAGE is narrow: a solved
        field is rounded once, when it is copied into its stack (its responses, ``synthetic``, are taken before that and
        are the bits of ``'double'``), and widened when a kernel loads it; weights, coefficients, sums and results are
        fp64 as before. Every kept value carries a relative error <= 2^-24, a product about 1e-7 of the sum of the
        magnitudes of its terms -- two orders of magnitude below the default ``tol_gradient`` the receiver fields are
        solved to. Rows of a stack are padded to a multiple of 16 B (``kept_bytes`` counts the padding). A value
        beyond the range of float32 (3.4e38) would become inf: ``forward()`` raises ``FloatingPointError``; values
        below its normal range (1.2e-38) lose digits or become 0, which is far below the rounding error of any product
        relative to its largest terms -- there is no per-field scaling."""

    def __init__(self, model, sources, frequencies, receivers, solver_opts=None, tol_gradient=1e-5, costs=None,
                 grids=None, interpolate_opts=None, magnetic=None, keep='device', batch=1, field_dtype='double'):
        if not (isinstance(field_dtype, str) and field_dtype in ('double', 'single')):
            raise ValueError(f"`field_dtype` must be 'double' or 'single'. Provided: {field_dtype!r}.")
        self.field_dtype = field_dtype
        super().__init__(model, sources, frequencies, receivers, solver_opts=solver_opts, tol_gradient=tol_gradient,
                         costs=costs, grids=grids, interpolate_opts=interpolate_opts, magnetic=magnetic, keep=keep,
                         batch=batch)
        if not self.keep:
            raise ValueError("`keep` must be 'device' or 'host' for ReciprocalSensitivity: without kept fields there "
                             f"is nothing to be solve-free from. Provided: {keep!r}.")
        if self.world > 1:
            raise NotImplementedError("ReciprocalSensitivity runs in one process; sharding frequencies over the ranks "
                                      f"of a process group (here: {self.world}) is not implemented.")
        shared = {}
        for sname, fname in self.pairs:
            g = self._grid_of((sname, fname))
            first = shared.setdefault(fname, g)
            if not (g is first or g == first):
                raise ValueError(f"ReciprocalSensitivity: all pairs of frequency {fname!r} must share one computational "
                                 f"grid (the receiver fields are shared by its sources); source {sname!r} has another.")
        if isinstance(self.grids, dict):         # equal meshes of a frequency: ONE object, one set of per-grid tables
            self.grids = {pair: shared[pair[1]] for pair in self.pairs}
        self.n_solves = {'forward': 0, 'receiver': 0, 'jvec': 0, 'jtvec': 0}
        self.setup_seconds = {'forward': 0.0, 'receiver': 0.0}

    def _reset(self):
        super()._reset()
        self._stacks = {}            # frequency name -> [source fields (ns x n), receiver fields (nr x n)]
        self._stage = None           # keep='host': the staging pair in HBM
        self._dchain = None
        self._widths = None          # the model grid's cell widths in HBM (regulariser)

    def __repr__(self):
        ns, nr, nf = len(self.sources), len(self._rec[0]), len(self.frequencies)
        held = sum(len(t) for st in self._stacks.values() for t in st)
        return (f"ReciprocalSensitivity: {len(self.pairs)} pairs ({ns} sources x {nf} frequencies), {nr * nf} receiver "
                f"fields ({nr} receivers x {nf} frequencies); keep={self.keep!r}, batch={self.batch}, "
                f"field_dtype={self.field_dtype!r}; kept fields: {held} "
                f"= {self.kept_bytes:,} B ({ {'device': 'HBM', 'host': 'pinned host memory'}[self.keep] })")

    @property
    def kept_bytes(self):
        """Bytes held by the kept source and receiver fields: (n_sources + n_receivers) x n_edges x 16 B per
        frequency (complex) with ``field_dtype='double'``; ``'single'``: x 8 B, every row padded to a multiple of
        16 B."""
        return int(sum(t.untyped_storage().nbytes() for st in self._stacks.values() for t in st))

    # ----------------------------------------------------------------------------- set-up ---
    def _new_stack(self, rows, n, dtype, dev):
        """A stack (rows, n) for solved fields of type ``dtype``. ``field_dtype='single'``: of the narrow partner type,
        a view of a (rows, stride) allocation whose rows start on 16-byte boundaries (full-width loads in
        ``emg3d_dev_sensitivity_dots_sp`` / ``_combine_sp``)."""
        import torch
        from emg3d_amd._device import free_hbm
        if self.field_dtype == 'single':
            dtype = {torch.complex128: torch.complex64, torch.float64: torch.float32}[dtype]
        size = torch.empty(0, dtype=dtype).element_size()
        stride = n if self.field_dtype == 'double' else -(-n * size // 16) * 16 // size
        if self.keep == 'host':
            return torch.empty((rows, stride), dtype=dtype, pin_memory=True)[:, :n]
        need, free = rows * stride * size, free_hbm(dev)
        if need > free:
            raise MemoryError(f"ReciprocalSensitivity: a stack of {rows} kept fields needs {need:,} B of HBM, "
                              f"{free:,} B are free; keep='host' holds the fields in pinned host memory instead.")
        return torch.empty((rows, stride), dtype=dtype, device=dev)[:, :n]

    def _receiver_chunks(self):
        """Receiver indices grouped for ``solve_batch`` under the rules of ``_chunks``."""
        nrec = len(self._rec[0])
        step = self.batch if self._may_batch() else 1
        return [list(range(r, min(r + step, nrec))) for r in range(0, nrec, step)]

    def forward(self):
        """The source solves at ``solver_opts['tol']`` (as ``Sensitivity``: same ``synthetic``), then the receiver
        solves at ``tol_gradient``, frequency by frequency; once -- later calls return at once."""
        if self._have_forward:
            return self
        import time
        import torch
        dev = self._device()
        nrec = len(self._rec[0])

        def lap(what=None, since=None):
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            if what:
                self.setup_seconds[what] += now - since
            return now
        opts = {**self.opts, 'tol': self.tol_gradient}
        for fname, freq in self.frequencies.items():
            mine = [i for i in self._order if self.pairs[i][1] == fname]
            if not mine:
                continue
            gkey, grid, gmodel, vol, plan = self._computational(self.pairs[mine[0]])
            n = grid.n_edges
            estack = xstack = None
            clock = lap()
            for row, i in enumerate(mine):
                e, self._synthetic[i] = self._solve_forward(i)
                if estack is None:
                    estack = self._new_stack(len(mine), n, e.dtype, dev)
                    xstack = self._new_stack(nrec, n, e.dtype, dev)
                    self._stacks[fname] = [estack, xstack]
                estack[row].copy_(e.to(estack.dtype))          # 'single': rounded here, once, on the device
                del e
            clock = lap('forward', clock)
            meta = Field(grid, frequency=freq)
            for chunk in self._receiver_chunks():
                rfields = []
                for r in chunk:
                    unit = np.full(nrec, np.nan, dtype=complex)
                    unit[r] = 1.0
                    rfields.append(residual_source_field(grid, freq, self.receivers, unit, np.ones(nrec), self._mag))
                back = self._solve_residual_sources(gkey, gmodel, meta, rfields, opts)
                for r, (field, info) in zip(chunk, back):
                    self.n_solves['receiver'] += 1
                    self.info[('receiver', r, fname)] = info
                    if field is None:                       # the solve failed: zero field, no contribution
                        xstack[r].zero_()
                    else:
                        xstack[r].copy_(field[:n].to(xstack.dtype))
                del back
            lap('receiver', clock)
            if self.field_dtype == 'single' and not all(bool(torch.isfinite(t).all()) for t in (estack, xstack)):
                del self._stacks[fname]
                raise FloatingPointError(
                    f"ReciprocalSensitivity: a kept field of frequency {fname!r} ({freq} Hz) is not finite in single "
                    "precision (an fp64 value beyond 3.4e38, or a solve that diverged); field_dtype='double' keeps the "
                    "fields as they are solved.")
        self._hier.clear()                   # the inner loop needs no hierarchy
        self._have_forward = True
        return self

    def _fields_of(self, fname):
        """The two stacks of a frequency in HBM (``keep='host'``: uploaded into the reused staging pair)."""
        import torch
        estack, xstack = self._stacks[fname]
        if self.keep == 'device':
            return estack, xstack
        if self._stage is None:
            dev = self._device()
            self._stage = [torch.empty(max(len(st[k]) * st[k].stride(0) for st in self._stacks.values()),
                                       dtype=estack.dtype, device=dev) for k in (0, 1)]
        return self._upload(self._stage, (estack, xstack))

    @staticmethod
    def _upload(bufs, hosts):
        """Pinned stacks into the flat HBM buffers ``bufs``, one contiguous copy each (rows with their padding, which
        no kernel reads); returns the (rows, n) views with the row stride of the host stacks."""
        out = []
        for buf, host in zip(bufs, hosts):
            rows, stride = len(host), host.stride(0)
            flat = buf[:rows * stride]
            flat.copy_(host.as_strided((rows * stride,), (1,), 0), non_blocking=False)
            out.append(flat.view(rows, stride)[:, :host.shape[1]])
        return out

    def _chain_factors(self, dev):
        """d sigma / d property of the model's own properties (n x n_cells in HBM, cells x fastest): the derivative
        chain of the mapping is a product with them, before G in ``jvec`` and after its transpose in ``jtvec``."""
        import torch
        if self._dchain is None:
            chain, shape = _DCHAIN[self.model.mapping], tuple(self.model.grid.shape_cells)
            self._dchain = torch.stack(self._cells_on_device(
                [chain(np.ones(shape), np.asarray(getattr(self.model, name), dtype=float))
                 for name in _PROPS[self.model.case]], dev))
        return self._dchain

    @staticmethod
    def _sp(stack):
        """Suffix of the C entry points for a stack: ``'_sp'`` for one stored in single precision, else ``''``."""
        import torch
        return '_sp' if stack.dtype in (torch.complex64, torch.float32) else ''

    def _entry(self, name, stack):
        """(the C entry point ``name`` for the storage type of ``stack``, its full name for ``_lib.check``)."""
        from emg3d_amd import _lib
        name += self._sp(stack)
        return getattr(_lib.lib(), name), name

    def _per_frequency(self):
        """(frequency name, pair indices, grid key, grid, cell volumes, averaging plan, s mu0) per frequency."""
        for fname, freq in self.frequencies.items():
            mine = [i for i in self._order if self.pairs[i][1] == fname]
            if mine:
                gkey, grid, gmodel, vol, plan = self._computational(self.pairs[mine[0]])
                yield fname, mine, gkey, grid, vol, plan, complex(Field(grid, frequency=freq).smu0)

    # ------------------------------------------------------------------------------- jvec ---
    def jvec(self, vector):
        """As ``Sensitivity.jvec``, without a solve: a block of one column through a ``_BlockPass`` -- per frequency
        one ``emg3d_dev_edge_weights`` and one ``emg3d_dev_sensitivity_dots_block``, which runs the single-vector kernel
        for one column."""
        v = _check_vector(self.model, vector)                   # raises on a wrong shape, before any GPU work
        dev = self._device()
        self.forward()
        jv = self._data_of(self._pass(dev, 1, 1).jvec(self._upload_block(v[None], dev)))
        return {pair: rows[0] for pair, rows in jv.items()}

    # ------------------------------------------------------------------------------ jtvec ---
    def jtvec(self, vector):
        """As ``Sensitivity.jtvec``, without a solve: one data set through a ``_BlockPass`` -- per frequency one
        ``emg3d_dev_sensitivity_combine_block``, which runs the single-vector kernel for one column, with the
        coefficients ``conj(vector)`` (0 for NaN or a missing pair) and one ``emg3d_dev_edges_to_cells``; the anisotropy
        bookkeeping and the derivative chain on the device, only the model's own components cross to the host."""
        self._check_data(vector)
        dev = self._device()
        self.forward()
        return self.from_device(self._gradient_block(self._pass(dev, 1, 1).jtvec([vector])))[0]

    def misfit_and_gradient(self, observed, weights=None):
        """Misfit ``sum w |synthetic - observed|^2 / 2`` from the kept responses and its gradient
        ``jtvec((synthetic - observed) w)``."""
        synthetic = self.synthetic
        misfit, data = 0.0, {}
        for i in self._order:
            pair = self.pairs[i]
            obs = np.asarray(observed[pair])
            w = np.ones(obs.shape) if weights is None else np.asarray(weights[pair], dtype=float)
            residual = synthetic[pair] - obs
            have = ~np.isnan(residual)
            misfit += float(np.sum(w[have] * (residual[have].conj() * residual[have])).real) / 2
            data[pair] = residual * w
        return misfit, self.jtvec(data)

    # ------------------------------------------------------------- Gauss-Newton Hessian ---
    def _check_weights(self, weights):
        """The data weights of ``misfit_and_gradient`` as dict pair -> (n_receivers,) floats for every pair: NaN or a
        missing pair count as 0, ``None`` as all ones; raises unless every entry is real, >= 0 and has one value per
        receiver."""
        nrec = len(self._rec[0])
        if weights is None:
            return {pair: np.ones(nrec) for pair in self.pairs}
        for pair, w in weights.items():
            if np.shape(w) != (nrec,):
                raise ValueError(f"`weights[{pair!r}]` must have shape ({nrec},): one value per receiver. "
                                 f"Provided: {np.shape(w)}.")
            if np.iscomplexobj(w) or np.any(np.asarray(w) < 0):
                raise ValueError(f"`weights[{pair!r}]` must be real and >= 0 (NaN: no datum). Provided: "
                                 f"{np.asarray(w).dtype} with minimum {np.nanmin(np.real(w))}.")
        return {pair: np.nan_to_num(np.asarray(weights[pair], dtype=float), nan=0.0) if pair in weights
                else np.zeros(nrec) for pair in self.pairs}

    def hessian_diagonal(self, weights=None):
        """Diagonal of the Gauss-Newton Hessian of the misfit ``sum w |r|^2 / 2``, ``diag Re(J^H W J)[c] = sum_i w_i
        |J_ic|^2`` -- the Jacobi preconditioner of a Gauss-Newton inner iteration, the pseudo-Hessian of a model update
        --, shaped and ordered like the result of ``jtvec``. ``weights``: dict (src, freq) -> real array (n_receivers)
        >= 0, as for ``misfit_and_gradient`` (NaN or a missing pair: 0; ``None``: all ones). Without a solve: per
        frequency one ``emg3d_dev_hessian_diagonal`` over the kept fields (a frequency whose weights are all zero is
        skipped). Every computational grid must be the model grid."""
        w = self._check_weights(weights)                        # raises before any GPU work
        self._require_model_grid('hessian_diagonal', 'before the modulus is taken')
        dev = self._device()
        self.forward()
        return self.from_device(self._hessian_diagonal_block(w, dev))[0]

    def _hessian_rows(self, entry, nrows, w, dev):
        """The frequency loop of ``hessian_diagonal`` and ``hessian_cell_blocks``: ``nrows`` rows of n_cells zeros in HBM
        into which one call of the C entry point ``entry`` (or its ``_sp`` sibling) per frequency accumulates, for the
        checked weights ``w``; a frequency whose weights are all zero is skipped. Without the chain factors."""
        import torch
        from emg3d_amd import _lib
        from emg3d_amd._device import _ptr, _stream
        rx, ry, rz = _EXPAND[self.model.case]
        ncell = self.model.grid.n_cells
        nx, ny, nz = self.model.grid.shape_cells
        h = torch.zeros(nrows * ncell, dtype=torch.float64, device=dev)
        for fname, mine, gkey, grid, vol, plan, smu0 in self._per_frequency():
            wf = np.stack([w[self.pairs[i]] for i in mine])
            if not wf.any():
                continue
            estack, xstack = self._fields_of(fname)
            wdev = torch.from_numpy(np.ascontiguousarray(wf)).to(dev)
            kernel, name = self._entry(entry, estack)
            _lib.check(kernel(
                nx, ny, nz, int(estack.is_complex()), _ptr(estack), estack.stride(0), len(estack),
                _ptr(xstack), xstack.stride(0), len(xstack), _ptr(wdev), rx, ry, rz, abs(smu0) ** 2, _ptr(vol), _ptr(h),
                ncell, _stream()), name)
        return h.view(nrows, ncell)

    def _hessian_diagonal_block(self, w, dev):
        """``hessian_diagonal`` for the checked weights ``w`` as a device block of one column, (1, n, n_cells)."""
        nrows = _NCOMP[self.model.case]
        d = self._chain_factors(dev)
        return self._hessian_rows('emg3d_dev_hessian_diagonal', nrows, w, dev)[None] * (d * d)

    @staticmethod
    def _packed_rows(n):
        """(p, q) of the packed rows of the cell blocks: the diagonal first, then (0,1), (0,2), (1,2)."""
        return [(p, p) for p in range(n)] + [(p, q) for q in range(1, n) for p in range(q)]

    def hessian_cell_blocks(self, weights=None, on_device=False):
        """The blocks of the Gauss-Newton Hessian ``Re(J^H W J)`` that couple the ``n`` properties of ONE cell:
        ``B[p, q, c] = sum_i w_i Re(conj(J_i[p, c]) J_i[q, c])``, shape ``(n, n) + shape_cells`` (cells ordered as
        ``jtvec`` orders them), symmetric bit for bit; its diagonal ``B[p, p]`` is ``hessian_diagonal``. It is the
        block-Jacobi preconditioner of a multi-parameter Gauss-Newton iteration (``gauss_newton_solve(precondition=
        'block')``) and a diagnostic: where ``B[p, q] / sqrt(B[p, p] B[q, q])`` is close to +-1 the data cannot
        separate the two properties. ``weights`` as for ``hessian_diagonal``. ``on_device=True``: the packed device
        tensor ``(n (n + 1) / 2, n_cells)`` instead, float64, rows (0,0) .. (n-1,n-1), then (0,1), (0,2), (1,2), cells
        x fastest. Without a solve: per frequency one ``emg3d_dev_hessian_cell_blocks`` over the kept fields, the same
        bytes as ``hessian_diagonal`` reads (a frequency whose weights are all zero is skipped). Every
        computational grid must be the model grid."""
        w = self._check_weights(weights)                        # raises before any GPU work
        self._require_model_grid('hessian_cell_blocks', 'before the product is taken')
        dev = self._device()
        self.forward()
        packed = self._hessian_cell_blocks_packed(w, dev)
        if on_device:
            return packed
        n, shape = _NCOMP[self.model.case], tuple(self.model.grid.shape_cells)
        rows = packed.cpu().numpy()
        out = np.empty((n, n) + shape, order='F')
        for m, (p, q) in enumerate(self._packed_rows(n)):
            out[p, q] = out[q, p] = rows[m].reshape(shape, order='F')
        return out

    def _hessian_cell_blocks_packed(self, w, dev):
        """``hessian_cell_blocks`` for the checked weights ``w``: the packed device tensor, row (p, q) times the chain
        factors ``d_p d_q``."""
        import torch
        n = _NCOMP[self.model.case]
        rows = self._packed_rows(n)
        d = self._chain_factors(dev)
        h = self._hessian_rows('emg3d_dev_hessian_cell_blocks', len(rows), w, dev)
        return h * torch.stack([d[p] * d[q] for p, q in rows])

    def hessian_vec(self, vector, weights=None):
        """Gauss-Newton Hessian times a model-shaped real ``vector``: ``jtvec({pair: weights[pair] * jvec(vector)[pair]})``,
        the product that ``hessian_diagonal`` preconditions, with its conventions for ``weights``."""
        w = self._check_weights(weights)                        # raises before any GPU work, as jvec does for `vector`
        jv = self.jvec(vector)
        return self.jtvec({pair: w[pair] * jv[pair] for pair in jv})

    # ------------------------------------------------------------- blocks of K vectors ---
    # A block of model vectors on the device: float64 (K, n, n_cells), n as for ``jvec`` (1, 2 or 3), cells x fastest --
    # ``jvec`` and ``jtvec`` are the products of a block of one.
    def _block_shapes(self):
        n, shape = _NCOMP[self.model.case], tuple(self.model.grid.shape_cells)
        return n, shape, [(n,) + shape] + ([shape] if n == 1 else [])

    def _check_vectors(self, vectors):
        """The NumPy block ``vectors``, K >= 1 model-shaped vectors as ``jvec`` takes them, as (K, n, nx, ny, nz)
        floats; raises unless it is real and every vector is shaped like the model's properties."""
        n, shape, allowed = self._block_shapes()
        v = np.asarray(vectors)
        if v.ndim < 1 or len(v) < 1 or v.shape[1:] not in allowed or np.iscomplexobj(v):
            raise ValueError(f"`vectors` must be real with shape (K,) + {' or (K,) + '.join(str(a) for a in allowed[::-1])}, "
                             f"K >= 1, for a model of case '{self.model.case}'. Provided: {v.dtype} {v.shape}.")
        return np.asarray(v, dtype=np.float64).reshape((len(v), n) + shape)

    def _check_device_block(self, block, dev=None):
        """Raises unless the tensor ``block`` is a device block of this instance: float64, (K >= 1, n, n_cells),
        contiguous, on a HIP device (``dev`` given: on that one)."""
        import torch
        n, ncell = _NCOMP[self.model.case], self.model.grid.n_cells
        if (block.dtype != torch.float64 or block.ndim != 3 or block.shape[0] < 1 or tuple(block.shape[1:]) != (n, ncell) or
                not block.is_contiguous() or block.device.type != 'cuda' or (dev is not None and block.device != dev)):
            raise ValueError(f"a device block must be a contiguous float64 tensor of shape (K, {n}, {ncell}), K >= 1, on "
                             f"the device of the fields{'' if dev is None else f' ({dev})'} for a model of case "
                             f"'{self.model.case}' (`to_device` builds one). Provided: {block.dtype} {tuple(block.shape)} on "
                             f"{block.device}, contiguous: {block.is_contiguous()}.")
        return block

    def _check_block(self, vectors):
        """``vectors`` of the block methods, validated without a device: (is a device block, the block)."""
        import torch
        if isinstance(vectors, torch.Tensor):
            return True, self._check_device_block(vectors)
        return False, self._check_vectors(vectors)

    @staticmethod
    def _check_columns(columns_per_pass):
        if isinstance(columns_per_pass, bool) or not isinstance(columns_per_pass, (int, np.integer)) or columns_per_pass < 1:
            raise ValueError(f"`columns_per_pass` must be an integer >= 1. Provided: {columns_per_pass!r}.")
        return int(columns_per_pass)

    def _upload_block(self, v, dev):
        import torch
        return torch.from_numpy(np.ascontiguousarray(v)).to(dev).permute(0, 1, 4, 3, 2).reshape(v.shape[0], v.shape[1], -1)

    def to_device(self, vectors):
        """The NumPy block ``vectors`` -- shape (K,) + a shape that ``jvec`` accepts, real, K >= 1 -- as a device block:
        float64 (K, n, n_cells) on the device of the fields, n = 1 (isotropic), 2 (HTI, VTI) or 3, cells x fastest.
        ``from_device`` is its inverse, exactly."""
        v = self._check_vectors(vectors)                        # raises before any GPU work
        return self._upload_block(v, self._device())

    def from_device(self, block):
        """The device block ``block`` as NumPy (K,) + the shape ``jtvec`` returns, every slice laid out like the result
        of ``jtvec``. ``to_device`` is its inverse, exactly."""
        self._check_device_block(block)
        n, shape, _ = self._block_shapes()
        K, rev = len(block), shape[::-1]
        if n == 1:
            return block.cpu().numpy().reshape((K,) + rev).transpose(0, 3, 2, 1)
        # (K, n_cells, n) in memory = component fastest, then x: the Fortran order of every (n, nx, ny, nz) slice
        return block.permute(0, 2, 1).contiguous().cpu().numpy().reshape((K,) + rev + (n,)).transpose(0, 4, 3, 2, 1)

    def _pass(self, dev, K, kc, weights=None):
        """A ``_BlockPass`` over the kept fields for K columns in groups of at most ``kc`` (``weights``: the checked data
        weights of its Hessian products): the engine of ``jvec`` and ``jtvec`` (a block of one column) and of the block
        methods, which use one for one product, and of ``gauss_newton_solve``, which keeps one for all its passes."""
        from emg3d_amd._blockpass import _BlockPass
        return _BlockPass(self, dev, K, kc, _EXPAND[self.model.case], weights)

    def _gradient_block(self, grad):
        """The bookkeeping of ``_finish_gradient``, the same operations in the same order, for the cell gradients (K, 3,
        n_cells) on the device: the device block (K, n, n_cells) of the model's own properties, of which ``from_device``
        downloads only those components, laid out as the result."""
        import torch
        case = self.model.case
        d = self._chain_factors(grad.device)
        rows = [grad[:, 0]]
        if case in ('HTI', 'triaxial'):
            rows.append(grad[:, 1] * d[1])
        else:
            rows[0] = rows[0] + grad[:, 1]
        if case in ('VTI', 'triaxial'):
            rows.append(grad[:, 2] * d[-1])
        else:
            rows[0] = rows[0] + grad[:, 2]
        rows[0] = rows[0] * d[0]
        return torch.stack(rows, dim=1)

    def _data_of(self, jv):
        """dict frequency name -> device (K, ns, nr) as dict pair -> NumPy (K, n_receivers): the one download."""
        out = {}
        for fname, mine, *_ in self._per_frequency():
            if fname in jv:
                res = jv[fname].cpu().numpy()
                for row, i in enumerate(mine):
                    out[self.pairs[i]] = res[:, row].copy()
        return {p: out[p] for p in self.pairs if p in out}

    def jvec_block(self, vectors, columns_per_pass=8):
        """``jvec`` for a block of K model vectors in one pass over the kept fields: dict (src, freq) -> complex array
        (K, n_receivers), real in the Laplace domain; row ``k`` is what ``jvec(vectors[k])`` returns (the sums run in
        another order: equal to rounding).

        ``vectors``: a NumPy block, shape (K,) + a shape ``jvec`` accepts, or a device block (``to_device``: float64
        (K, n, n_cells) on the device of the fields, cells x fastest); K >= 1. Per frequency the stacks are fetched once
        (``keep='host'``: ONE upload for the block), the derivative chain is one product on the block, then per group
        of at most ``columns_per_pass`` columns one ``emg3d_dev_edge_weights`` per column and one
        ``emg3d_dev_sensitivity_dots_block``; scratch: ``columns_per_pass x n_edges x 8 B``, allocated
        once per call (``MemoryError`` if that is not free). The only download is the result. No solve: ``n_solves``
        does not move."""
        kc = self._check_columns(columns_per_pass)
        on_dev, block = self._check_block(vectors)              # raises on a wrong block, before any GPU work
        dev = self._device()
        self.forward()
        block = self._check_device_block(block, dev) if on_dev else self._upload_block(block, dev)
        return self._data_of(self._pass(dev, len(block), kc).jvec(block))

    def _check_data_block(self, data):
        if isinstance(data, dict) or not hasattr(data, '__len__') or len(data) < 1:
            raise ValueError("`data` must be a sequence of K >= 1 data dictionaries (src, freq) -> (n_receivers,) values, "
                             f"as `jtvec` takes them. Provided: {type(data).__name__}"
                             f"{'' if isinstance(data, dict) or not hasattr(data, '__len__') else ' of length 0'}.")
        data = list(data)
        for vector in data:
            self._check_data(vector)
        return data

    def jtvec_block(self, data, on_device=False, columns_per_pass=8):
        """``jtvec`` for K data sets in one pass over the kept fields: NumPy (K,) + the shape ``jtvec`` returns, slice
        ``k`` the bits of ``jtvec(data[k])``; ``on_device=True``: the device block (K, n, n_cells) instead (see
        ``jvec_block``; ``from_device`` converts it), nothing is downloaded.

        ``data``: a sequence of K >= 1 data dictionaries as ``jtvec`` takes them (NaN or a missing pair: no datum). Per
        frequency the stacks are fetched once, then per group of at most ``columns_per_pass`` columns one
        ``emg3d_dev_sensitivity_combine_block`` and one ``emg3d_dev_edges_to_cells`` per column; the anisotropy
        bookkeeping and the derivative chain run on the block. Scratch: ``columns_per_pass x n_edges x 16 B`` (Laplace
        domain: 8 B), allocated once per call (``MemoryError`` if that is not free). No solve."""
        kc = self._check_columns(columns_per_pass)
        data = self._check_data_block(data)                     # raises before any GPU work
        dev = self._device()
        self.forward()
        out = self._gradient_block(self._pass(dev, len(data), kc).jtvec(data))
        return out if on_device else self.from_device(out)

    def hessian_vec_block(self, vectors, weights=None, on_device=None, columns_per_pass=8):
        """``hessian_vec`` for a block of K model vectors, ``J^H W J`` applied to every column, with the data left on the
        device: per frequency the stacks are fetched once, ``emg3d_dev_sensitivity_dots_block`` gives jv (K, ns, nr),
        the coefficients ``conj(weights * jv)`` are formed there and go straight into
        ``emg3d_dev_sensitivity_combine_block`` -- no download, no upload and no wait between the two halves.

        ``vectors``: as for ``jvec_block``; a device block gives a device block (``on_device=None``), a NumPy block
        NumPy as ``jtvec_block`` returns it; ``on_device`` True / False decides otherwise. ``weights``: as for
        ``hessian_diagonal``. Slice ``k`` equals ``hessian_vec(vectors[k], weights)`` to rounding. Scratch: both of
        ``jvec_block`` and ``jtvec_block``."""
        kc = self._check_columns(columns_per_pass)
        w = self._check_weights(weights)                        # raises before any GPU work, as do the next two
        on_dev, block = self._check_block(vectors)
        dev = self._device()
        self.forward()
        block = self._check_device_block(block, dev) if on_dev else self._upload_block(block, dev)
        out = self._gradient_block(self._pass(dev, len(block), kc, w).hessian_vec(block))
        return out if (on_dev if on_device is None else on_device) else self.from_device(out)

    # ------------------------------------------------ orthonormal blocks and the truncated SVD ---
    _MAX_BLOCK = 64          # columns of emg3d_dev_block_gram / emg3d_dev_block_rotate

    def _check_block_columns(self, K, what):
        if K > self._MAX_BLOCK:
            raise ValueError(f"{what} must not exceed {self._MAX_BLOCK}, the widest block of `emg3d_dev_block_gram`. "
                             f"Provided: {K}.")

    def _orthonormaliser(self, dev, kmax):
        from emg3d_amd._blockpass import _BlockOrth
        return _BlockOrth(dev, kmax, _NCOMP[self.model.case] * self.model.grid.n_cells)

    def orthonormalise_block(self, vectors, on_device=None):
        """An orthonormal basis of the span of K <= 64 model vectors, in the Euclidean inner product of the vectors as
        ``jtvec`` returns them: ``(Q, rank)``, ``Q`` with ``rank <= K`` columns -- fewer when the vectors are
        numerically dependent. ``vectors`` and the form of ``Q`` as for ``hessian_vec_block``: a NumPy block gives
        NumPy, a device block a device block (which is left as it is), ``on_device`` True / False decides otherwise; a
        block of zeros gives ``rank`` 0 and an empty block of the same form, (0, n, n_cells) on the device.

        Gram-based SVQB, applied twice: per application ``emg3d_dev_block_gram``, the K x K matrix on
        the host (scaled to a unit diagonal, ``eigh``, directions below ``K eps`` times the largest eigenvalue dropped)
        and ``emg3d_dev_block_rotate``. No Cholesky: a sketch of a sensitivity has a Gram matrix whose condition is the
        square of an already fast decay. Scratch: one second block. Neither ``forward()`` nor the kept fields are
        needed."""
        on_dev, block = self._check_block(vectors)              # raises before any GPU work
        self._check_block_columns(len(block), 'the number of `vectors`')
        dev = self._device()
        block = self._check_device_block(block, dev).clone() if on_dev else self._upload_block(block, dev).contiguous()
        K, n, ncell = block.shape
        q, rank = self._orthonormaliser(dev, K)(block.view(K, n * ncell))
        to_dev = on_dev if on_device is None else on_device
        if rank == 0:
            return (block[:0] if to_dev else np.zeros((0,) + self._block_shapes()[2][0])), 0
        q = q.view(rank, n, ncell)
        return (q if to_dev else self.from_device(q)), rank

    def sensitivity_svd(self, rank, weights=None, oversample=8, power_iterations=1, seed=0, on_device=False,
                        columns_per_pass=8):
        """Truncated singular value decomposition of the weighted sensitivity ``A = W^1/2 J^`` by the randomised range
        finder of Halko, Martinsson and Tropp: ``A ~ U diag(s) V^T``. ``J^`` (M, N) has the rows ``Re J_i`` and ``Im J_i``
        in the ordering of ``stack_data``, with the derivative chain of the mapping -- the matrix of ``data_gram`` --,
        ``W`` the ``weights`` (as for ``hessian_diagonal``), repeated for the two rows of a datum.

        Returns ``U`` (M, k) float64 with orthonormal columns, ``s`` (k,) descending, and ``V``: k model vectors shaped
        like the result of ``jtvec``, NumPy (k,) + that shape or, ``on_device=True``, the device block (k, n, n_cells).
        ``k <= rank``; it is smaller when the sketch is numerically rank-deficient (fewer data with a weight than
        ``rank``). The entry of largest magnitude of every column of ``U`` (the first of them) is positive. It gives the
        step of a truncated pseudo-inverse, the model resolution ``V V^T``, posterior variances, the effective rank of
        a survey.

        With ``l = min(rank + oversample, M)`` <= 64: ``Omega`` (M, l) standard normal from
        ``numpy.random.default_rng(seed)`` on the host -- the result is a function of the arguments alone --, ``Y = J^T
        W^1/2 Omega`` by the pass of ``jtvec_block``, ``Q = orth(Y)`` (``orthonormalise_block``), ``power_iterations``
        times ``Q = orth(J^T W J Q)`` by the pass of ``hessian_vec_block``, ``B = W^1/2 J^ Q`` (M, l') by the pass of
        ``jvec_block``, its thin SVD on the host, ``V = Q W_B`` by ``emg3d_dev_block_rotate``. ``2 +
        2 power_iterations`` half passes over the kept fields whatever M is, through ONE pass object; nothing of
        length N crosses the host but the final ``V`` with ``on_device=False``. Other computational grids (``grids=``)
        are served as by the block products. Frequency-domain surveys only. No solve: ``n_solves`` does not move.

        Accuracy: a power iteration works on the squares of the singular values, and its orthonormalisation drops what
        falls below ``sqrt(l eps)`` of the largest. Singular values below about 1e-4 of ``s[0]`` come back less accurate
        with ``power_iterations >= 1``, or not at all (``k`` smaller). Where the small end of the spectrum matters and
        ``rank + oversample`` reaches M, ``power_iterations=0`` is exact to rounding."""
        rank = self._check_count('rank', rank)                  # everything is validated before any GPU work
        for name, value in (('oversample', oversample), ('power_iterations', power_iterations), ('seed', seed)):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 0:
                raise ValueError(f"`{name}` must be an integer >= 0. Provided: {value!r}.")
        w = self._check_weights(weights)
        kc = self._check_columns(columns_per_pass)
        if {float(f) < 0 for f in self.frequencies.values()} != {False}:
            raise NotImplementedError("sensitivity_svd: frequency-domain surveys only; in the Laplace domain `jvec` is minus "
                                      "the adjoint of `jtvec` (see `data_gram`): the passes do not form J^T W J there.")
        nrec = len(self._rec[0])
        M = 2 * len(self.pairs) * nrec
        ell = min(rank + int(oversample), M)
        self._check_block_columns(ell, 'min(`rank` + `oversample`, M)')
        dev = self._device()
        self.forward()
        n, ncell = _NCOMP[self.model.case], self.model.grid.n_cells
        root_w = np.tile(np.sqrt(np.concatenate([w[pair] for pair in self.pairs])), 2)
        omega = np.random.default_rng(int(seed)).standard_normal((M, ell))
        ps = self._pass(dev, ell, kc, w)
        orth = self._orthonormaliser(dev, ell)

        def orthonormal(grad):
            q, r = orth(self._gradient_block(grad).view(len(grad), n * ncell))
            if 0 < r < ps.K:
                ps.shrink(r)
            return q.view(r, n, ncell), r
        q, r = orthonormal(ps.jtvec([self.unstack_data(root_w * omega[:, j]) for j in range(ell)]))
        for _ in range(int(power_iterations)):
            if r == 0:
                break
            q, r = orthonormal(ps.hessian_vec(q))
        if r == 0:                                              # A = 0 to rounding: no datum carries a weight
            return (np.zeros((M, 0)), np.zeros(0),
                    q.view(0, n, ncell) if on_device else np.zeros((0,) + self._block_shapes()[2][0]))
        jq = self._data_of(ps.jvec(q))
        B = np.stack([root_w * self.stack_data({pair: jq[pair][j] for pair in jq}) for j in range(r)], axis=1)
        U, s, Wt = np.linalg.svd(B, full_matrices=False)
        k = min(rank, r)
        U, s, Wb = np.ascontiguousarray(U[:, :k]), s[:k].copy(), Wt[:k].T
        top = np.argmax(np.abs(U), axis=0)                      # (the first of equal magnitudes)
        sign = np.where(U[top, np.arange(k)] < 0, -1.0, 1.0)
        V = orth.rotate(q.view(r, n * ncell), Wb * sign[None, :]).view(k, n, ncell)
        return U * sign[None, :], s, V.clone() if on_device else self.from_device(V)

    # ------------------------------------------- regulariser and the inner Gauss-Newton solve ---
    @staticmethod
    def _check_dampings(dampings):
        """``dampings`` as a float64 array (K,), K >= 1; raises unless it is 1-D, real, finite and > 0."""
        lam = np.asarray(dampings)
        if (lam.ndim != 1 or lam.size < 1 or lam.dtype.kind not in 'fiu' or not np.all(np.isfinite(lam)) or
                not np.all(lam > 0)):
            raise ValueError("`dampings` must be a 1-D sequence of K >= 1 finite values > 0. "
                             f"Provided: {lam.dtype} {lam.shape}"
                             f"{'' if lam.size > 8 or lam.ndim != 1 else ' ' + str(lam.tolist())}.")
        return np.ascontiguousarray(lam, dtype=np.float64)

    @staticmethod
    def _check_regulariser(smallness, smoothness):
        """(alpha_s, alpha_x, alpha_y, alpha_z) as floats; raises unless all are finite and >= 0 and one is > 0."""
        sm = np.asarray(smoothness)
        if sm.shape != (3,) or sm.dtype.kind not in 'fiu' or not np.all(np.isfinite(sm)) or not np.all(sm >= 0):
            raise ValueError("`smoothness` must be three finite values >= 0 (alpha_x, alpha_y, alpha_z). "
                             f"Provided: {smoothness!r}.")
        if (isinstance(smallness, bool) or not isinstance(smallness, (int, float, np.integer, np.floating)) or
                not np.isfinite(smallness) or smallness < 0):
            raise ValueError(f"`smallness` must be a finite value >= 0. Provided: {smallness!r}.")
        if smallness == 0 and not sm.any():
            raise ValueError("`smallness` and `smoothness` must not all be zero: the regulariser would be the zero "
                             f"operator. Provided: smallness={smallness!r}, smoothness={smoothness!r}.")
        return (float(smallness),) + tuple(float(a) for a in sm)

    def _check_active(self, active):
        """``active`` as a bool array shaped like the cells, or None."""
        if active is None:
            return None
        a, shape = np.asarray(active), tuple(self.model.grid.shape_cells)
        if a.dtype != bool or a.shape != shape:
            raise ValueError(f"`active` must be a bool array of shape {shape}, one value per cell. "
                             f"Provided: {a.dtype} {a.shape}.")
        return a

    def _check_irls(self, cell_weights, norms, linearise_at, irls_eps):
        """The weighted / sparse-norm arguments of the regulariser, validated without a device. None if all four are
        None; otherwise (weights, norms, u, eps): weights NumPy (1 or n, n_cells) with cells x fastest, a tensor as given
        or None; norms four floats; u NumPy (n, n_cells), a tensor as given or None; eps two floats (0 without u)."""
        import torch
        if cell_weights is None and norms is None and linearise_at is None and irls_eps is None:
            return None
        n, shape, allowed = self._block_shapes()
        ncell = self.model.grid.n_cells

        def rows(a):
            return np.stack([c.ravel(order='F') for c in a.reshape((-1,) + shape)])

        def tensor_ok(t, shapes):
            return t.dtype == torch.float64 and tuple(t.shape) in shapes and t.is_contiguous() and t.device.type == 'cuda'
        w = cell_weights
        if isinstance(w, torch.Tensor):
            if not tensor_ok(w, [(ncell,), (n, ncell)]):
                raise ValueError(f"`cell_weights` on the device must be a contiguous float64 tensor of shape ({ncell},) or "
                                 f"({n}, {ncell}). Provided: {w.dtype} {tuple(w.shape)} on {w.device}, contiguous: "
                                 f"{w.is_contiguous()}.")
        elif w is not None:
            a = np.asarray(w)
            if (a.dtype.kind not in 'fiu' or a.shape not in (shape, (n,) + shape) or not np.all(np.isfinite(a)) or
                    not np.all(a >= 0)):
                raise ValueError(f"`cell_weights` must be real, finite and >= 0 with shape {shape} (one array for all "
                                 f"components) or {(n,) + shape}. Provided: {a.dtype} {a.shape}.")
            w = rows(np.asarray(a, dtype=np.float64))
        ps = (2.0, 2.0, 2.0, 2.0)
        if norms is not None:
            a = np.asarray(norms)
            if a.shape != (4,) or a.dtype.kind not in 'fiu' or not np.all(np.isfinite(a)) or not np.all((a >= 0) & (a <= 2)):
                raise ValueError("`norms` must be four finite values in [0, 2] (p_s, p_x, p_y, p_z). "
                                 f"Provided: {norms!r}.")
            ps = tuple(float(p) for p in a)
        sparse = any(p != 2.0 for p in ps)
        u, eps = linearise_at, (0.0, 0.0)
        if not sparse and (u is not None or irls_eps is not None):
            raise ValueError("`linearise_at` and `irls_eps` belong to norms other than 2: with all four norms 2 they would "
                             f"be ignored. Provided: norms={norms!r}, linearise_at "
                             f"{'given' if u is not None else 'None'}, irls_eps={irls_eps!r}.")
        if sparse:
            if u is None or irls_eps is None:
                raise ValueError("a norm other than 2 needs `linearise_at` (the deviation m - m_ref at which the weights "
                                 f"are frozen) and `irls_eps`. Provided: norms={norms!r}, linearise_at "
                                 f"{'given' if u is not None else 'None'}, irls_eps={irls_eps!r}.")
            if isinstance(u, torch.Tensor):
                if not tensor_ok(u, [(n, ncell)]):
                    raise ValueError(f"`linearise_at` on the device must be a contiguous float64 tensor of shape ({n}, "
                                     f"{ncell}). Provided: {u.dtype} {tuple(u.shape)} on {u.device}, contiguous: "
                                     f"{u.is_contiguous()}.")
            else:
                a = np.asarray(u)
                if a.dtype.kind not in 'fiu' or a.shape not in allowed or not np.all(np.isfinite(a)):
                    raise ValueError("`linearise_at` must be one real, finite model-shaped vector of shape "
                                     f"{' or '.join(str(s) for s in allowed[::-1])}. Provided: {a.dtype} {a.shape}.")
                u = rows(np.asarray(a, dtype=np.float64))
            a = np.asarray(irls_eps)
            if a.shape != (2,) or a.dtype.kind not in 'fiu' or not np.all(np.isfinite(a)) or not np.all(a > 0):
                raise ValueError("`irls_eps` must be two finite values > 0 (eps_s, eps_g). "
                                 f"Provided: {irls_eps!r}.")
            eps = tuple(float(e) for e in a)
        return w, ps, u, eps

    def _upload_irls(self, irls, dev):
        """The result of ``_check_irls`` with its arrays in HBM (uploads come before kernels), or None."""
        import torch
        if irls is None:
            return None

        def up(a, name):
            if a is None or not isinstance(a, torch.Tensor):
                return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            if a.device != dev:
                raise ValueError(f"`{name}` must be on the device of the fields ({dev}). Provided: on {a.device}.")
            return a
        w, ps, u, eps = irls
        return up(w, 'cell_weights'), ps, up(u, 'linearise_at'), eps

    @staticmethod
    def _irls_args(irls, ncell):
        """The C arguments between ``mask`` and ``nvec`` of the weighted entries."""
        from emg3d_amd._device import _ptr
        w, ps, u, eps = irls
        wstride = ncell if w is not None and w.ndim == 2 and w.shape[0] > 1 else 0
        return (None if w is None else _ptr(w), wstride, None if u is None else _ptr(u), 0 if u is None else ncell) + ps + eps

    @staticmethod
    def _check_count(name, value):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
            raise ValueError(f"`{name}` must be an integer >= 1. Provided: {value!r}.")
        return int(value)

    def _check_rhs(self, rhs, K):
        """``rhs`` of ``gauss_newton_solve``, validated without a device: (is on the device, is ONE vector for all
        columns, the block -- NumPy (K or 1, n, nx, ny, nz) or the tensor as given)."""
        import torch
        n, shape, allowed = self._block_shapes()
        ncell = self.model.grid.n_cells
        if isinstance(rhs, torch.Tensor):
            if rhs.ndim == 2:
                self._check_device_block(rhs[None])
                return True, True, rhs[None]
            block = self._check_device_block(rhs)
        else:
            v = np.asarray(rhs)
            if v.shape in allowed and not np.iscomplexobj(v):
                return False, True, np.asarray(v, dtype=np.float64).reshape((1, n) + shape)
            try:
                block = self._check_vectors(rhs)
            except ValueError as e:
                raise ValueError(str(e).replace('`vectors`', '`rhs`')) from None
        if len(block) != K:
            raise ValueError(f"`rhs` must be one model-shaped vector or a block of K = len(dampings) = {K} vectors. "
                             f"Provided: a block of {len(block)} ({n} x {ncell} cells each).")
        return isinstance(rhs, torch.Tensor), False, block

    def _regulariser_geometry(self, active, dev):
        """(nx, ny, nz, device widths hx, hy, hz, device mask as uint8 with cells x fastest or None)."""
        import torch
        if self._widths is None or self._widths[0].device != dev:
            self._widths = [torch.from_numpy(np.ascontiguousarray(h, dtype=np.float64)).to(dev) for h in self.model.grid.h]
        mask = None
        if active is not None:
            mask = torch.from_numpy(np.ascontiguousarray(active.ravel(order='F').astype(np.uint8))).to(dev)
        return tuple(self.model.grid.shape_cells) + tuple(self._widths) + (mask,)

    def _regulariser(self, geo, alphas, p, q, beta=0.0, lam=None, pq=None, ws=None, irls=None):
        """One ``emg3d_dev_model_regulariser`` on the device blocks ``p`` -> ``q``; with ``irls`` (of ``_upload_irls``)
        one ``emg3d_dev_model_regulariser_weighted``."""
        from emg3d_amd import _lib
        from emg3d_amd._device import _ptr, _stream
        nx, ny, nz, hx, hy, hz, mask = geo
        K, n, ncell = p.shape
        mask, lam, pq, wsp = (None if t is None else _ptr(t) for t in (mask, lam, pq, ws))
        if irls is not None:
            _lib.check(_lib.lib().emg3d_dev_model_regulariser_weighted(
                nx, ny, nz, _ptr(hx), _ptr(hy), _ptr(hz), *alphas, mask, *self._irls_args(irls, ncell), K * n, n, _ptr(p),
                _ptr(q), beta, lam, pq, wsp, 0 if ws is None else ws.numel(), _stream()),
                'emg3d_dev_model_regulariser_weighted')
            return q
        _lib.check(_lib.lib().emg3d_dev_model_regulariser(
            nx, ny, nz, _ptr(hx), _ptr(hy), _ptr(hz), *alphas, mask, K * n, n, _ptr(p), _ptr(q), beta, lam, pq, wsp,
            0 if ws is None else ws.numel(), _stream()), 'emg3d_dev_model_regulariser')
        return q

    def regulariser_vec_block(self, vectors, smallness=0.0, smoothness=(1.0, 1.0, 1.0), active=None, on_device=None, *,
                              cell_weights=None, norms=None, linearise_at=None, irls_eps=None):
        """The model regulariser ``R`` applied to a block of K model vectors, every component of every vector on its
        own: the finite-volume smallness-plus-roughness operator on the model grid,

            (R v)[c] = a[c] (smallness V_c v[c] + sum_d smoothness[d] sum_{faces f of c along d} a[c'] A_f / l_f (v[c] - v[c']))

        with the cell volume ``V_c``, the face area ``A_f``, the distance ``l_f`` of the two cell centres and the mask
        ``a`` = ``active`` (bool, shaped like the cells; ``None``: all cells). Faces on the boundary of the grid and
        towards an inactive cell are left out (Neumann), rows of inactive cells are 0; ``R`` is symmetric positive
        semi-definite and annihilates constants exactly when ``smallness`` is 0. It acts on the model's own parameters,
        whatever the mapping.

        ``vectors`` and ``on_device``: as for ``hessian_vec_block`` (a device block gives a device block). One
        ``emg3d_dev_model_regulariser`` for the block; neither forward fields nor a solve are needed.
        With it a user forms right-hand sides such as ``-(g + lambda R (m - m_ref))`` for ``gauss_newton_solve``.

        The weighted / sparse-norm form (keyword only, all ``None``: the operator above through the same entry point
        as ever; otherwise ``emg3d_dev_model_regulariser_weighted``). Component ``k`` of a vector has
        cell weights ``w_k`` and linearisation values ``u_k``, the same for all K vectors:

            (R v)[c] = a[c] (cs[c] v[c] + sum_f cf[c,f] (v[c] - v[c']))
            cs[c]    = smallness V_c w[c] rho(p_s, eps_s; u[c])
            cf[c,f]  = smoothness[d] a[c'] (A_f / l_f) (w[c] + w[c']) / 2 rho(p_d, eps_g; (u[c] - u[c']) / l_f)
            rho(p, eps; t) = (t^2 + eps^2)^(p / 2 - 1), exactly 1 for p = 2

        cell_weights: real, finite, >= 0, shaped like the cells (one array for all components) or like a model vector
            ``(n, nx, ny, nz)`` -- depth or sensitivity weighting, for example a power of ``hessian_diagonal()``; or a
            float64 device tensor ``(n_cells,)`` / ``(n, n_cells)``, cells x fastest. ``None``: 1.
        norms: ``(p_s, p_x, p_y, p_z)`` in [0, 2], the measures of the deviation and of its three gradients in their
            lagged-diffusivity (IRLS, Ekblom) form. ``None``: all 2.
        linearise_at: one model-shaped real vector (NumPy, or a device tensor ``(n, n_cells)``): the deviation
            ``m - m_ref`` of the model's own parameters at which the weights ``rho`` are frozen. Needed exactly when a
            norm is not 2; given with all norms 2 it raises, so that nothing is silently ignored.
        irls_eps: ``(eps_s, eps_g)``, both > 0; needed exactly when a norm is not 2.

        ``R`` stays symmetric (as stored, bit for bit) positive semi-definite and annihilates constants when
        ``smallness`` is 0. The outer IRLS loop is the user's: it updates ``linearise_at``, cools ``irls_eps`` and
        handles the reference model; one call is one frozen linearisation."""
        import torch
        alphas = self._check_regulariser(smallness, smoothness)     # raises before any GPU work, as do the next three
        mask = self._check_active(active)
        irls = self._check_irls(cell_weights, norms, linearise_at, irls_eps)
        on_dev, block = self._check_block(vectors)
        dev = self._device()
        block = self._check_device_block(block, dev) if on_dev else self._upload_block(block, dev)
        irls = self._upload_irls(irls, dev)
        out = self._regulariser(self._regulariser_geometry(mask, dev), alphas, block, torch.empty_like(block), irls=irls)
        return out if (on_dev if on_device is None else on_device) else self.from_device(out)

    def _regulariser_diagonal(self, geo, alphas, irls, dev):
        """diag R on the device: (n_cells,) from ``emg3d_dev_model_regulariser_diagonal``, shared by the components, or,
        with ``irls`` (of ``_upload_irls``), (n, n_cells) from ``emg3d_dev_model_regulariser_weighted_diagonal``."""
        import torch
        from emg3d_amd import _lib
        from emg3d_amd._device import _ptr, _stream
        L = _lib.lib()
        n, ncell = _NCOMP[self.model.case], self.model.grid.n_cells
        nx, ny, nz, hx, hy, hz, dmask = geo
        if irls is None:
            rd = torch.empty(ncell, dtype=torch.float64, device=dev)
            _lib.check(L.emg3d_dev_model_regulariser_diagonal(
                nx, ny, nz, _ptr(hx), _ptr(hy), _ptr(hz), *alphas, None if dmask is None else _ptr(dmask), _ptr(rd),
                _stream()), 'emg3d_dev_model_regulariser_diagonal')
        else:                                                   # one diagonal of R per component
            rd = torch.empty((n, ncell), dtype=torch.float64, device=dev)
            _lib.check(L.emg3d_dev_model_regulariser_weighted_diagonal(
                nx, ny, nz, _ptr(hx), _ptr(hy), _ptr(hz), *alphas, None if dmask is None else _ptr(dmask),
                *self._irls_args(irls, ncell), n, _ptr(rd), _stream()), 'emg3d_dev_model_regulariser_weighted_diagonal')
        return rd

    @staticmethod
    def _check_data_rank(data_rank):
        if data_rank is None:
            return None
        if isinstance(data_rank, bool) or not isinstance(data_rank, (int, np.integer)) or data_rank < 1:
            raise ValueError(f"`data_rank` must be None or an integer >= 1. Provided: {data_rank!r}.")
        return int(data_rank)

    def _require_data_preconditioner(self):
        """Raises unless ``precondition='data'`` can serve this survey: the limits of ``data_gram``, without a device."""
        what = "gauss_newton_solve(precondition='data')"
        self._require_model_grid(what, 'before the product is taken')
        if self._data_rows() != 2:
            raise NotImplementedError(f"{what}: frequency-domain surveys only; in the Laplace domain `jvec` is minus the "
                                      "adjoint of `jtvec` (see `data_gram`) and the identity behind the preconditioner "
                                      "changes its signs.")

    def _data_preconditioner_setup(self, dev, w, rd, dmask, data_rank):
        """The set-up of the data-space preconditioner from the checked weights ``w``, the device
        diagonal ``rd`` of R ((n_cells,) or (n, n_cells)) and the device mask: ``dinv`` = 1 / rd on active cells (1 where
        rd is not positive, 0 on inactive cells), ``G0 = J^ diag(dinv) J^T`` by ``_data_gram_block``, ``s`` = the square
        roots of the weights in the ordering of ``stack_data``, and on the host, in fp64, ``eigh`` of ``B = diag(s) G0
        diag(s)``: negative eigenvalues are set to 0 and the ``min(data_rank, M)`` largest pairs kept. A dict: in HBM
        ``dinv`` (rows ``dinv_stride`` apart), ``q`` (M, rank), ``eigenvalues`` (rank, descending), ``s`` (M) and per
        frequency with a weight > 0 the positions ``index[name] = (Re, Im)`` of its data in the stacked vector; on the
        host ``q_host``, ``eigenvalues_host`` (all M, descending, clipped), ``s_host``; ``n_data``, ``rank``; ``seconds``
        of the four steps gram / download / eigh / upload."""
        import time
        import torch
        n, ncell = _NCOMP[self.model.case], self.model.grid.n_cells
        nrec, npair = len(self._rec[0]), len(self.pairs)

        def lap(since=None):
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            return now if since is None else (now, now - since)
        seconds = {}
        clock = lap()
        rows = rd.view(-1, ncell)
        dinv = torch.where(rows > 0, 1.0 / rows, torch.ones_like(rows))
        if dmask is not None:
            dinv = torch.where(dmask != 0, dinv, torch.zeros_like(dinv))
        dinv = dinv.contiguous()
        d = self._chain_factors(dev)
        G0 = self._data_gram_block((dinv.expand(n, ncell) * (d * d)).contiguous(), 2, dev)
        clock, seconds['gram'] = lap(clock)
        G0 = G0.cpu().numpy()
        clock, seconds['download'] = lap(clock)
        s = np.sqrt(np.tile(np.concatenate([w[pair] for pair in self.pairs]), 2))
        M = len(s)
        rank = M if data_rank is None else min(data_rank, M)
        eig, Q = np.linalg.eigh(s[:, None] * G0 * s[None, :])
        eig, Q = np.maximum(eig[::-1], 0.0), Q[:, ::-1]
        q_host, eig_host = np.ascontiguousarray(Q[:, :rank]), np.ascontiguousarray(eig[:rank])
        clock, seconds['eigh'] = lap(clock)
        index = {}
        for fname, mine, *_ in self._per_frequency():
            if np.stack([w[self.pairs[i]] for i in mine]).any():
                re = torch.tensor([i * nrec + r for i in mine for r in range(nrec)], dtype=torch.int64, device=dev)
                index[fname] = (re, re + npair * nrec)
        up = [torch.from_numpy(a).to(dev) for a in (q_host, eig_host, s)]
        clock, seconds['upload'] = lap(clock)
        return {'dinv': dinv, 'dinv_stride': ncell if len(dinv) > 1 else 0, 'q': up[0], 'eigenvalues': up[1], 's': up[2],
                'index': index, 'n_data': M, 'rank': rank, 'q_host': q_host, 'eigenvalues_host': eig, 's_host': s,
                'seconds': seconds}

    def _data_preconditioner(self, dampings, weights=None, smallness=0.0, smoothness=(1.0, 1.0, 1.0), active=None,
                             data_rank=None, columns_per_pass=8, *, cell_weights=None, norms=None, linearise_at=None,
                             irls_eps=None):
        """The data-space preconditioner of ``gauss_newton_solve(precondition='data')`` on its own, arguments as there:
        ``(setup, apply)`` with the dict of ``_data_preconditioner_setup`` and ``apply(block)``, which returns ``M_k
        block[k]`` for the K = ``len(dampings)`` columns of a device block as a new device block, through the kernels
        and the pass of the solve."""
        import torch
        kc = self._check_columns(columns_per_pass)
        lam = self._check_dampings(dampings)
        alphas = self._check_regulariser(smallness, smoothness)
        mask = self._check_active(active)
        irls = self._check_irls(cell_weights, norms, linearise_at, irls_eps)
        data_rank = self._check_data_rank(data_rank)
        w = self._check_weights(weights)
        self._require_data_preconditioner()
        dev = self._device()
        self.forward()
        K, n, ncell = len(lam), _NCOMP[self.model.case], self.model.grid.n_cells
        pcg = self._pcg(dev, torch.zeros((K, n, ncell), dtype=torch.float64, device=dev), lam, kc, w,
                        self._regulariser_geometry(mask, dev), alphas, self._upload_irls(irls, dev), 'data', data_rank)

        def apply(block):
            r = self._check_device_block(block, dev)
            if len(r) != K:
                raise ValueError(f"the block must have K = len(dampings) = {K} columns. Provided: {len(r)}.")
            pcg.r.copy_(r)
            return pcg.precondition(1).clone()
        return pcg.pre, apply

    def _pcg(self, dev, r, lam, kc, w, geo, alphas, irls, precondition, data_rank=None, tol=0.0):
        """The ``_BlockPCG`` of ``gauss_newton_solve`` for the device residual block ``r`` (K, n, n_cells) after the
        set-up of its preconditioner -- ``precondition``: ``'data'``, ``'block'`` (block-Jacobi: the packed cell blocks
        and diag R; one component per cell: Jacobi), True (Jacobi: the two diagonals) or False --, on a new
        ``_BlockPass``: every buffer of the iteration is allocated here, behind the temporaries of the set-up. (``tol``
        is read by the scalar step alone.)"""
        from emg3d_amd._blockpass import _BlockPCG
        hd = rd = pre = None
        blocks = precondition == 'block' and r.shape[1] > 1
        if precondition == 'data':
            pre = self._data_preconditioner_setup(dev, w, self._regulariser_diagonal(geo, alphas, irls, dev), geo[6], data_rank)
        elif blocks:
            hd = self._hessian_cell_blocks_packed(w, dev).contiguous()
            rd = self._regulariser_diagonal(geo, alphas, irls, dev)
        elif precondition:
            hd = self._hessian_diagonal_block(w, dev)[0].contiguous()
            rd = self._regulariser_diagonal(geo, alphas, irls, dev)
        return _BlockPCG(self._pass(dev, len(lam), kc, w), lam, r, tol, geo[6], (hd, rd), irls is not None, pre, blocks)

    def gauss_newton_solve(self, rhs, dampings, weights=None, smallness=0.0, smoothness=(1.0, 1.0, 1.0), active=None,
                           tol=1e-3, maxit=50, precondition=True, check_every=4, on_device=None, columns_per_pass=8, *,
                           cell_weights=None, norms=None, linearise_at=None, irls_eps=None, data_rank=None):
        """The inner linear solve of a Gauss-Newton step for K dampings at once: column ``k`` solves

            (Re(J^H W J) + dampings[k] R) x_k = b_k

        by preconditioned conjugate gradients, from ``x_k = 0`` until ``|r_k| <= tol |b_k|`` (``b_k`` masked by
        ``active``; 2-norms over all components). The K iterations are independent but share every operator
        application: ``H p`` is ONE ``hessian_vec_block`` pass over the kept fields for all columns, everything else a
        few fused kernels on the device blocks. Returns ``(x, info)``.

        rhs: one model-shaped vector, used for every column, or a block of K = ``len(dampings)`` vectors; NumPy as
            ``jvec_block`` takes them, or on the device (a block (K, n, n_cells) of ``to_device``; one vector: (n,
            n_cells)). ``x`` is NumPy ``(K,) +`` the shape ``jtvec`` returns, or a device block if ``rhs`` is on the
            device; ``on_device`` True / False decides otherwise.
        dampings: K >= 1 finite values > 0. weights: as for ``hessian_diagonal``.
        smallness, smoothness, active: the regulariser ``R`` of ``regulariser_vec_block``. Inactive cells are taken
            out of the system: their entries of ``x`` are exactly 0.
        cell_weights, norms, linearise_at, irls_eps (keyword only): the weighted / sparse-norm form of ``R``, as for
            ``regulariser_vec_block``: ``R`` becomes the seven-point operator whose coefficients carry the cell weights
            and the IRLS weights ``(t^2 + eps^2)^(p / 2 - 1)`` frozen at ``linearise_at``. They are
            uploaded once, before the first kernel; the Jacobi preconditioner then takes the diagonal of ``R`` per
            component. All ``None``: the entry points and the bits of the plain operator. The outer IRLS loop --
            updating ``linearise_at``, cooling ``irls_eps``, the reference model -- is the user's, as is the rest of
            the inversion.
        precondition: Jacobi, ``1 / (hessian_diagonal(weights) + dampings[k] diag R)``, formed inside the kernels from
            the two diagonals, which all columns share (where that sum is not positive: 1). Needs every computational
            grid to be the model grid, as ``hessian_diagonal`` does. False: no preconditioner. ``'block'``: block-Jacobi
            (DESIGN.md 4.20): per cell the inverse of the ``n x n`` block ``hessian_cell_blocks(weights)[:, :, c] +
            dampings[k] diag R``, by a Cholesky factorisation in registers inside the kernels
            (``emg3d_dev_pcg_update_blk`` / ``_direction_blk``); a cell whose block is not positive definite in floating
            point takes the Jacobi rule. It removes the cross-talk of the properties of one cell (sigma_h and sigma_v of
            VTI), which Jacobi ignores; the set-up is one pass over the kept fields, as for Jacobi, and the limits are
            Jacobi's. A model with one property per cell (``n = 1``) takes the Jacobi route itself. ``'data'``: the data-space
            (Woodbury) preconditioner. ``H = J^T W J`` has rank at most M, the number of real data, so
            ``(lambda_k diag R + H)^-1`` is ``diag R^-1 / lambda_k`` minus a correction through an M x M matrix: once
            per call ``data_gram(1 / diag R)`` is formed, scaled by the square roots of the weights and decomposed on the
            host (``numpy.linalg.eigh``, fp64) -- ONE decomposition serves all K dampings, which only change the filter
            ``lambda_k / (lambda_k + eigenvalue)``. It is exact when ``R`` is diagonal (smallness only: one iteration);
            otherwise only the off-diagonal part of ``lambda R`` is left to the iteration. An application is one more
            block pass over the kept fields (``emg3d_dev_pcg_scale``, ``dots_block``, ``emg3d_dev_data_space_filter``,
            ``combine_block``, ``emg3d_dev_pcg_finish``; then ``emg3d_dev_pcg_direction_z``), so an iteration costs
            about twice a Jacobi one. It has the limits of ``data_gram``: every computational grid must be the model
            grid, frequency-domain surveys only; the set-up costs ``eigh`` of an M x M matrix on the host.
        data_rank (keyword only; ignored unless ``precondition='data'``): ``None`` or an integer >= 1: keep only the
            ``min(data_rank, M)`` largest eigenpairs. The preconditioner is then the exact inverse of ``lambda_k diag R``
            plus the rank-``data_rank`` part of ``H``: symmetric positive definite for every rank, and PCG needs about one
            more iteration per eigenvalue left out.
        check_every: the host reads the table of the per-column scalars (64 B per column) every so many iterations --
            the only download inside the loop -- and stops when no column is running, or at ``maxit``. A column that
            has stopped is frozen ON THE DEVICE: its ``x`` keeps its bits however long the others run, so the result
            does not depend on ``check_every``, bit for bit; the passes after the last column has stopped are wasted.

        info: ``iterations`` (K,), ``relative_residual`` (K,) ``|r_k| / |b_k|`` of the recurrence, ``state`` (K,) -- 0
        stopped by ``maxit``, 1 converged, 2 breakdown (``<p, (H + lambda R) p> <= 0``), 3 a sum was not finite --,
        ``history`` (list of (K,) relative residuals, one per look at the table, the one after the set-up first),
        ``hessian_passes`` (``H p`` passes only), ``preconditioner_passes`` (application passes of ``'data'``, one more
        than the former for the set-up; otherwise 0) and ``data_rank`` (the rank used; otherwise ``None``); with
        ``'data'`` also ``setup_seconds`` of the preconditioner: gram / download / eigh / upload.

        The weights are uploaded once and one set of scratch buffers serves all passes. ``keep='host'``: every pass
        uploads the two stacks of every frequency again, as every block product does -- ``kept_bytes`` over PCIe per
        iteration, and an application pass of ``'data'`` uploads them twice, once for each of its halves;
        ``keep='device'`` is the mode this method is meant for. No solve: ``n_solves`` does not move."""
        kc = self._check_columns(columns_per_pass)              # everything is validated before any GPU work
        lam = self._check_dampings(dampings)
        alphas = self._check_regulariser(smallness, smoothness)
        mask = self._check_active(active)
        irls = self._check_irls(cell_weights, norms, linearise_at, irls_eps)
        if isinstance(tol, bool) or not isinstance(tol, (float, np.floating)) or not 0 < tol < 1:
            raise ValueError(f"`tol` must be a float in (0, 1). Provided: {tol!r}.")
        maxit, check_every = self._check_count('maxit', maxit), self._check_count('check_every', check_every)
        w = self._check_weights(weights)
        K = len(lam)
        on_dev, single, b = self._check_rhs(rhs, K)
        by_data = isinstance(precondition, str) and precondition == 'data'
        by_block = isinstance(precondition, str) and precondition == 'block'
        if by_data:
            data_rank = self._check_data_rank(data_rank)
            self._require_data_preconditioner()
        elif by_block:
            self._require_model_grid("gauss_newton_solve(precondition='block')", 'before the product is taken')
        elif precondition:
            self._require_model_grid('gauss_newton_solve(precondition=True)', 'before the modulus is taken')
        dev = self._device()
        self.forward()
        n, ncell = _NCOMP[self.model.case], self.model.grid.n_cells
        b = self._check_device_block(b, dev) if on_dev else self._upload_block(b, dev)
        irls = self._upload_irls(irls, dev)
        geo = self._regulariser_geometry(mask, dev)
        pcg = self._pcg(dev, (b.expand(K, n, ncell) if single else b).clone(), lam, kc, w, geo, alphas, irls,
                        'data' if by_data else 'block' if by_block else bool(precondition), data_rank, tol)

        def look():
            t = pcg.table.cpu().numpy()
            with np.errstate(invalid='ignore', divide='ignore'):
                rel = np.where(t[:, 1] > 0, np.sqrt(t[:, 5] / t[:, 1]), 0.0)
            history.append(rel)
            return t, rel
        history, passes = [], 0
        pcg.step(1)
        t, rel = look()
        for it in range(1, maxit + 1):
            if not np.any(t[:, 7] == 0):
                break
            q = self._gradient_block(pcg.ps.hessian_vec(pcg.p))
            passes += 1
            self._regulariser(geo, alphas, pcg.p, q, beta=1.0, lam=pcg.lam, pq=pcg.pq, ws=pcg.rws, irls=irls)
            pcg.step(0, q)
            if it % check_every == 0 or it == maxit:
                t, rel = look()
        info = {'iterations': t[:, 6].astype(int), 'relative_residual': rel, 'state': t[:, 7].astype(int),
                'history': history, 'hessian_passes': passes, 'preconditioner_passes': passes + 1 if by_data else 0,
                'data_rank': pcg.pre['rank'] if by_data else None}
        if by_data:
            info['setup_seconds'] = pcg.pre['seconds']
        return (pcg.x if (on_dev if on_device is None else on_device) else self.from_device(pcg.x)), info

    # ------------------------------------------------------- data-space normal matrix ---
    def _data_rows(self):
        """Real rows per datum in ``data_gram``: 2 (frequency domain: Re and Im) or 1 (Laplace domain); a survey that
        mixes the two is refused."""
        laplace = {float(f) < 0 for f in self.frequencies.values()}
        if len(laplace) > 1:
            raise NotImplementedError("data_gram: the survey mixes Laplace- and frequency-domain frequencies; their "
                                      "kept fields have different types (real and complex).")
        return 1 if laplace == {True} else 2

    def stack_data(self, data):
        """The data dictionary ``data`` (pair -> (n_receivers,) values, as ``jtvec`` takes it) as the real vector
        (M,) in the ordering of ``data_gram``: datum ``i = pair index * n_receivers + receiver`` (pairs as in
        ``self.pairs``), entry ``i`` its real part and, in the frequency domain, entry ``N + i`` its imaginary part.
        NaN or a missing pair: 0. Host code: neither a GPU nor ``forward()`` is needed."""
        nrec, c = self._check_data(data), self._data_rows()
        n = len(self.pairs) * nrec
        out = np.zeros(c * n)
        for i, pair in enumerate(self.pairs):
            y = data.get(pair)
            if y is not None:
                y = np.array(y, dtype=complex)
                y[np.isnan(y)] = 0.0
                out[i * nrec:(i + 1) * nrec] = y.real
                if c == 2:
                    out[n + i * nrec:n + (i + 1) * nrec] = y.imag
        return out

    def unstack_data(self, vector):
        """The inverse of ``stack_data`` on complete data: dict pair -> (n_receivers,) complex values (Laplace
        domain: real values) of a real vector (M,)."""
        nrec, c = len(self._rec[0]), self._data_rows()
        n = len(self.pairs) * nrec
        v = np.asarray(vector)
        if v.shape != (c * n,) or np.iscomplexobj(v):
            raise ValueError(f"`vector` must be real with shape ({c * n},): {c} x {len(self.pairs)} pairs x {nrec} "
                             f"receivers. Provided: {v.dtype} {v.shape}.")
        v = np.asarray(v, dtype=np.float64)
        return {pair: (v[i * nrec:(i + 1) * nrec] + 1j * v[n + i * nrec:n + (i + 1) * nrec] if c == 2
                       else v[i * nrec:(i + 1) * nrec].copy()) for i, pair in enumerate(self.pairs)}

    def _check_model_weights(self, model_weights):
        """The model weights of ``data_gram`` as (n, nx, ny, nz) floats (``None``: ones); raises unless they are real,
        >= 0 and shaped like the vector of ``jvec``."""
        if model_weights is None:
            return np.ones((_NCOMP[self.model.case],) + tuple(self.model.grid.shape_cells))
        try:
            m = _check_vector(self.model, model_weights)
        except ValueError as e:
            raise ValueError(str(e).replace('`vector`', '`model_weights`')) from None
        if not np.all(m >= 0):
            raise ValueError(f"`model_weights` must be >= 0. Provided: minimum {np.min(m)}"
                             f"{', with NaN' if np.isnan(m).any() else ''}.")
        return m

    def data_gram(self, model_weights=None):
        """The data-space Gauss-Newton matrix ``J^ diag(model_weights) J^T``: ndarray (M, M) of float64, C-contiguous
        and exactly symmetric, in the ordering of ``stack_data`` -- ``J^`` has the rows ``Re J_i`` and (frequency
        domain) ``Im J_i`` of the sensitivity of ``jtvec(y) = sum_i Re(conj(y_i) J_i)``, so for all data y, z

            stack_data(y) @ G @ stack_data(z) == sum(model_weights * jtvec(y) * jtvec(z))
            G @ stack_data(y)                 == stack_data(jvec(model_weights * jtvec(y)))

        (the second in the frequency domain; in the Laplace domain ``jvec`` is MINUS the adjoint of ``jtvec``, as in the
        reference, and the right-hand side changes its sign -- the matrix is positive semi-definite in both).

        ``model_weights``: real, >= 0, shaped like the vector of ``jvec`` (``None``: ones). Without a solve and
        without ever forming ``J^``: one ``emg3d_dev_data_gram`` over the kept fields per unordered pair of
        frequencies, the transposed block is copied; assembled on the device, downloaded once.
        ``keep='host'`` holds a second staging pair for the duration of the call when there is more than one
        frequency. Every computational grid must be the model grid."""
        import torch
        m = self._check_model_weights(model_weights)            # raises before any GPU work
        self._require_model_grid('data_gram', 'before the product is taken')
        c = self._data_rows()
        dev = self._device()
        self.forward()
        d = self._chain_factors(dev)
        mw = (torch.from_numpy(np.ascontiguousarray(m)).to(dev).permute(0, 3, 2, 1).reshape(len(m), -1) * (d * d)).contiguous()
        return self._data_gram_block(mw, c, dev).cpu().numpy()

    def _data_gram_block(self, mw, c, dev):
        """``data_gram`` on the device: ``mw`` holds the model weights times the squared chain factors, contiguous
        float64 (n, n_cells) in HBM; ``c`` = ``_data_rows()``. Returns the matrix (M, M) in HBM."""
        import torch
        from emg3d_amd import _lib
        from emg3d_amd._device import _ptr, _stream
        L = _lib.lib()
        rx, ry, rz = _EXPAND[self.model.case]
        ncell = self.model.grid.n_cells
        nx, ny, nz = self.model.grid.shape_cells
        nrec = len(self._rec[0])
        n = len(self.pairs) * nrec
        G = torch.zeros((c * n, c * n), dtype=torch.float64, device=dev)
        per_freq = list(self._per_frequency())
        # rows of G of a frequency's block: Re of its data (its pairs in the order of its stack), then Im
        rows = [torch.tensor([part * n + i * nrec + r for part in range(c) for i in mine for r in range(nrec)],
                             dtype=torch.int64, device=dev) for _, mine, *_ in per_freq]
        second = None                                           # keep='host': staging pair of the partner frequency
        try:
            for a, (fa, mine_a, _, _, vol, _, smu0_a) in enumerate(per_freq):
                ea, xa = self._fields_of(fa)
                is_complex = int(ea.is_complex())
                kernel, name = self._entry('emg3d_dev_data_gram', ea)
                for b in range(a, len(per_freq)):
                    fb, mine_b, _, _, _, _, smu0_b = per_freq[b]
                    if b == a:
                        eb, xb = ea, xa
                    elif self.keep == 'device':
                        eb, xb = self._stacks[fb]
                    else:
                        if second is None:
                            second = [torch.empty_like(buf) for buf in self._stage]
                        eb, xb = self._upload(second, self._stacks[fb])
                    na, nb = len(mine_a) * nrec, len(mine_b) * nrec
                    ws_len = L.emg3d_data_gram_ws_len(nx, ny, nz, is_complex, na, nb)
                    ws = torch.empty(ws_len, dtype=torch.float64, device=dev)
                    blk = torch.empty((c * na, c * nb), dtype=torch.float64, device=dev)
                    _lib.check(kernel(
                        nx, ny, nz, is_complex, _ptr(ea), ea.stride(0), len(ea), _ptr(xa), xa.stride(0), len(xa),
                        smu0_a.real, smu0_a.imag, _ptr(eb), eb.stride(0), len(eb), _ptr(xb), xb.stride(0), len(xb),
                        smu0_b.real, smu0_b.imag, rx, ry, rz, _ptr(mw), ncell, _ptr(vol), _ptr(blk), c * nb, _ptr(ws),
                        ws_len, _stream()), name)
                    G[rows[a][:, None], rows[b][None, :]] = blk
                    if b != a:
                        G[rows[b][:, None], rows[a][None, :]] = blk.T
                    del ws, blk
        finally:
            del second
        return G


def jvec(model, vector, sources, frequencies, receivers, **kwargs):
    """One-shot ``Sensitivity(model, sources, frequencies, receivers, **kwargs).jvec(vector)``."""
    lin = Sensitivity(model, sources, frequencies, receivers, **kwargs)
    try:
        return lin.jvec(vector)
    finally:
        lin.release()


def jtvec(model, vector, sources, frequencies, receivers, **kwargs):
    """One-shot ``Sensitivity(model, sources, frequencies, receivers, **kwargs).jtvec(vector)``."""
    lin = Sensitivity(model, sources, frequencies, receivers, **kwargs)
    try:
        return lin.jtvec(vector)
    finally:
        lin.release()
