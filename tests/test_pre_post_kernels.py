"""The kernels before and after a solve, one C-ABI call at a time and past one workgroup: ``emg3d_dev_magnetic_field``,
``_volume_average``, ``_linear_eval``, ``_spline_filter`` / ``_spline_eval`` (``csrc/receivers.h``) and
``emg3d_dev_source_field``, ``_volume_model`` (second half of ``csrc/adjoint.h``), and the methods on top of them.

All but the spline kernels launch 64 x 4 x 1 threads (one plane per ``blockIdx.z``) or 64 threads per block, so the
shapes put 63, 64, 65 and 130 cells along x and 3, 4, 5 and 9 along y, more than 64 segments into a wire and more
than 64 points into an interpolation; ``test_every_kernel_runs_past_one_block`` states which case does it per kernel.

References: the curl, the volume average and the volume model are written out below in NumPy in ``longdouble`` /
``clongdouble`` from the mathematics of the operation (their own rounding, 2^-64, is far below every bound); the two
restatements that have reference vectors under ``tests/golden/`` first prove themselves against them without a GPU.
The interpolation kernels are compared with SciPy, the source kernel with the host ``get_source_field`` and with a
conservation law that no implementation enters.

Criteria: derived, not tuned. ``u = eps / 2`` is the unit roundoff; a bound is a counted number of roundings times the
sum of the MAGNITUDES of the terms (of the factors where two products can cancel); every docstring gives its count.
The device's ``pow``, ``exp`` and ``log10`` enter with the maximum error that the OpenCL C specification (section
"Relative error as ULPs", double precision) requires of them and that the ROCm device library is written to meet:
pow <= 16 ulp, exp <= 3 ulp, log10 <= 3 ulp (one ulp is at most eps = 2 u relative). The SciPy comparisons keep the
suite's 1e-12 absolute for N(0, 1) data.

Doubles go to the device in one buffer with a NaN behind every array (``_fence``), outputs that a kernel must write
start as NaN, and outputs have a guard element behind every component that must survive.
"""
import functools

import numpy as np
import pytest

import emg3d_amd as emg3d
from emg3d_amd import _lib, models
from emg3d_amd.fields import EPSILON_0
from test_reciprocal import _dev, _up
from test_sensitivity import EPS, MU_0, _stretched, record

U = EPS / 2                         # unit roundoff
LD, CLD = np.longdouble, np.clongdouble
EDGE = [(1, 1, 1), (63, 3, 2), (64, 4, 1), (65, 5, 3), (130, 9, 2)]
GUARD = 7.5


def _ratio(diff, bound):
    """Worst |diff| / bound over the entries with a positive bound (0 if there is none)."""
    m = bound > 0
    return float(np.max(diff[m] / bound[m])) if np.any(m) else 0.0


# ------------------------------------------------------------------- NumPy restatements ---
def curl_numpy(e3, zeta, h, smu0, mag=False):
    """H on the faces from E on the edges, (mx, my, mz) with shapes (nx+1, ny, nz), (nx, ny+1, nz), (nx, ny, nz+1):
    forward differences of the edge components over the cell widths, times (zeta_lower + zeta_upper) / (s mu0) over
    ((h_lower + h_upper) times the two transverse widths) on the interior faces; both boundary faces of every
    component are zero. ``mag``: the same expression with every factor replaced by its magnitude and every difference
    by a sum -- what the bounds are relative to."""
    cplx = np.iscomplexobj(e3[0]) or np.iscomplexobj(smu0)
    ex, ey, ez = (np.abs(c).astype(LD) if mag else c.astype(CLD if cplx else LD) for c in e3)
    hx, hy, hz = (np.asarray(w, dtype=LD) for w in h)
    hx, hy, hz = hx[:, None, None], hy[None, :, None], hz[None, None, :]
    z = np.asarray(zeta).astype(LD)
    f = 1 / (CLD(smu0) if cplx else LD(np.real(smu0)))
    f = np.abs(f).astype(LD) if mag else f
    d = (lambda a, b: a + b) if mag else (lambda a, b: a - b)
    cx = d(d(ez[:, 1:], ez[:, :-1]) / hy, d(ey[:, :, 1:], ey[:, :, :-1]) / hz)
    cy = d(d(ex[:, :, 1:], ex[:, :, :-1]) / hz, d(ez[1:], ez[:-1]) / hx)
    cz = d(d(ey[1:], ey[:-1]) / hx, d(ex[:, 1:], ex[:, :-1]) / hy)
    mx, my, mz = np.zeros_like(cx), np.zeros_like(cy), np.zeros_like(cz)
    mx[1:-1] = cx[1:-1] * (z[:-1] + z[1:]) * f / ((hx[:-1] + hx[1:]) * hy * hz)
    my[:, 1:-1] = cy[:, 1:-1] * (z[:, :-1] + z[:, 1:]) * f / (hx * (hy[:, :-1] + hy[:, 1:]) * hz)
    mz[:, :, 1:-1] = cz[:, :, 1:-1] * (z[:, :, :-1] + z[:, :, 1:]) * f / (hx * hy * (hz[:, :, :-1] + hz[:, :, 1:]))
    return mx, my, mz


def overlap(x_in, x_out):
    """O[o, i]: length of the overlap of output cell o with input cell i along one axis; the first and the last input
    cell extend to -inf / +inf (the nearest extrapolation)."""
    x_in, x_out = np.asarray(x_in, dtype=LD), np.asarray(x_out, dtype=LD)
    lo, hi = x_in[:-1].copy(), x_in[1:].copy()
    lo[0], hi[-1] = -np.inf, np.inf
    return np.maximum(0, np.minimum(x_out[1:, None], hi[None]) - np.maximum(x_out[:-1, None], lo[None]))


def _nodes(grid):
    return grid.nodes_x, grid.nodes_y, grid.nodes_z


def _volumes(grid):
    hx, hy, hz = (np.asarray(w, dtype=LD) for w in grid.h)
    return hx[:, None, None] * hy[None, :, None] * hz[None, None, :]


def overlaps(grid, new_grid):
    return [overlap(a, b) for a, b in zip(_nodes(grid), _nodes(new_grid))]


def volume_average_numpy(grid, new_grid, v, log):
    """sum over the input cells of overlap volume times value, over the output cell's volume; ``log``: of log10(value),
    and 10 ** of the result."""
    v = np.asarray(v).astype(LD)
    a = np.einsum('ai,bj,ck,ijk->abc', *overlaps(grid, new_grid), np.log10(v) if log else v) / _volumes(new_grid)
    return LD(10) ** a if log else a


def conductivity_numpy(p, mapping):
    p = np.asarray(p).astype(LD)
    return {'Conductivity': lambda: p, 'Resistivity': lambda: 1 / p, 'LgConductivity': lambda: LD(10) ** p,
            'LgResistivity': lambda: LD(10) ** -p, 'LnConductivity': lambda: np.exp(p),
            'LnResistivity': lambda: np.exp(-p)}[mapping]()


def s_value(frequency):
    """s = 2 pi i f (f > 0) or -f (f < 0), in extended precision (pi: the double that everybody uses)."""
    return CLD(1j) * (2 * LD(np.pi) * LD(frequency)) if frequency > 0 else LD(-frequency)


# ----------------------------------------------------------------------- not gpu tests ---
@pytest.mark.parametrize('tag', ['f', 's'])
def test_curl_restatement_vs_reference_vectors(golden_receivers, tag):
    """``curl_numpy`` against the reference's magnetic fields (12 x 10 x 8, mu_r, frequency and Laplace domain with
    s = -frequency): 1e-14 of the largest entry."""
    g = golden_receivers
    grid = emg3d.TensorMesh([g['hx'], g['hy'], g['hz']], g['origin'])
    freq = float(g[tag + '_frequency'])
    e = emg3d.Field(grid, data=g[tag + '_efield'], frequency=freq)
    zeta = _volumes(grid) / g['mu_r'].astype(LD)
    smu0 = s_value(freq) * LD(float(g['meta_mu_0']))
    got = np.concatenate([c.ravel('F') for c in curl_numpy((e.fx, e.fy, e.fz), zeta, grid.h, smu0)])
    want = g[tag + '_hfield']
    rel = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    record(f"curl_numpy vs golden {tag}_hfield: max |diff| / max |want| = {rel:.2e}")
    assert got.shape == want.shape and np.iscomplexobj(got) == np.iscomplexobj(want)
    assert rel <= 1e-14


@pytest.mark.parametrize('mapping', ['Resistivity', 'Conductivity', 'LgConductivity'])
def test_volume_average_restatement_vs_reference_vectors(golden_gridding, mapping):
    """``volume_average_numpy`` against every re-gridded property of the reference (finer, coarser and beyond the
    input, shared nodes): 1e-14 of the largest entry. The log rule is that of ``interpolate_to_grid``: on a log10
    scale unless the mapping is logarithmic already, for the properties; ``mu_r`` and ``epsilon_r`` go with it."""
    g = golden_gridding
    mesh = lambda t: emg3d.TensorMesh([g[f'{t}_hx'], g[f'{t}_hy'], g[f'{t}_hz']], g[f'{t}_origin'])   # noqa: E731
    log = not mapping.startswith('L')
    worst = 0.0
    for t in ('fine', 'coarse', 'same_nodes'):
        for p in ('property_x', 'property_z', 'mu_r', 'epsilon_r'):
            got = volume_average_numpy(mesh('in'), mesh(t), g[f'{mapping}_in_{p}'], log)
            want = g[f'{mapping}_{t}_{p}']
            rel = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
            worst = max(worst, rel)
            assert got.shape == want.shape and rel <= 1e-14, (t, p, rel)
    record(f"volume_average_numpy vs golden {mapping}: max |diff| / max |want| = {worst:.2e}")


# ------------------------------------------------------------------------ device helpers ---
def _fence(*arrays):
    """One device tensor that holds the arrays with a NaN behind each, and their element offsets."""
    dtype = np.result_type(*arrays)
    parts, offsets, n = [], [], 0
    for a in arrays:
        a = np.asarray(a, dtype=dtype).ravel()
        offsets.append(n)
        parts += [a, np.full(1, np.nan, dtype=dtype)]
        n += a.size + 1
    return _up(np.concatenate(parts)), offsets


def _guarded(sizes, dtype, fill):
    """Output components of ``sizes`` elements filled with ``fill``, a GUARD behind each: (tensor, offsets)."""
    import torch
    offsets = np.cumsum([0] + [s + 1 for s in sizes])
    t = torch.full((int(offsets[-1]),), fill, dtype=dtype, device=_dev())
    for o, s in zip(offsets, sizes):
        t[int(o) + s] = GUARD
    return t, [int(o) for o in offsets[:-1]]


def _split(t, offsets, shapes):
    """The components (F-order) of a guarded tensor; the guards must have survived."""
    a = t.cpu().numpy()
    out = []
    for o, sh in zip(offsets, shapes):
        n = int(np.prod(sh))
        assert a[o + n] == GUARD, "the element behind an output component was overwritten"
        out.append(a[o:o + n].reshape(sh, order='F'))
    return out


def _field3(rng, shapes, is_complex):
    return [rng.standard_normal(sh) + (1j * rng.standard_normal(sh) if is_complex else 0) for sh in shapes]


# --------------------------------------------------------------------- k_edge_curl ---
@pytest.mark.gpu
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('shape', EDGE)
def test_magnetic_field_kernel_vs_numpy(shape, is_complex):
    """``emg3d_dev_magnetic_field`` entry by entry against ``curl_numpy`` within 12 eps times ``curl_numpy(mag=True)``
    -- the magnitudes of the FACTORS: the two differences of a curl component can cancel. Outputs start as NaN: every
    face must come back finite, both boundary planes of every component exactly 0, the guards untouched.

    Count, real field, in u: a difference (1), the reciprocal width (1) and their product (1) per term, the difference
    of the two terms (1): 4 on the curl; zeta_lower + zeta_upper (1), 1 / (s mu0) (1), their product (1): 3; the sum of
    two widths (1), two products (2), the reciprocal (1): 4; two final products (2): 13 u = 6.5 eps. Complex field:
    the component-wise 4 u of the curl are sqrt(2) 4 u on the modulus, 1 / (s mu0) as conj / |.|^2 has 5, its product
    with the real sum 1 + 1, the complex product sqrt(5) u (Brent et al.), the real factor 4 + 1:
    5.7 + 7 + 2.3 + 5 = 20 u = 10 eps. 12 eps covers both."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    grid = _stretched(*shape)
    nx, ny, nz = shape
    rng = np.random.default_rng(sum(shape) + is_complex)
    eshapes = (grid.shape_edges_x, grid.shape_edges_y, grid.shape_edges_z)
    fshapes = (grid.shape_faces_x, grid.shape_faces_y, grid.shape_faces_z)
    e3 = _field3(rng, eshapes, is_complex)
    mu_r = rng.uniform(0.7, 3.0, shape)
    zeta = (grid.cell_volumes.reshape(shape, order='F') / mu_r)
    smu0 = 2j * np.pi * 0.7 * MU_0 if is_complex else 0.7 * MU_0
    E, eo = _fence(*[c.ravel('F') for c in e3])
    G, go = _fence(zeta.ravel('F'), *grid.h)
    out, oo = _guarded([int(np.prod(s)) for s in fshapes], E.dtype, float('nan'))
    _lib.check(_lib.lib().emg3d_dev_magnetic_field(
        nx, ny, nz, int(is_complex), _ptr(E, eo[0]), _ptr(E, eo[1]), _ptr(E, eo[2]), _ptr(G, go[0]), _ptr(G, go[1]),
        _ptr(G, go[2]), _ptr(G, go[3]), complex(smu0).real, complex(smu0).imag, _ptr(out, oo[0]), _ptr(out, oo[1]),
        _ptr(out, oo[2]), _stream()), 'emg3d_dev_magnetic_field')
    torch.cuda.synchronize()
    got = _split(out, oo, fshapes)
    want = curl_numpy(e3, zeta, grid.h, smu0)
    mag = curl_numpy(e3, zeta, grid.h, smu0, mag=True)
    worst = 0.0
    for axis, (g, w, m) in enumerate(zip(got, want, mag)):
        assert g.dtype == (np.complex128 if is_complex else np.float64)
        assert np.all(np.isfinite(g)), f"component {axis}: a face was not written"
        lower, upper = np.take(g, 0, axis=axis), np.take(g, -1, axis=axis)
        assert not np.any(lower) and not np.any(upper), f"component {axis}: a boundary plane is not zero"
        diff, bound = np.abs(g - w).astype(float), (12 * EPS * m).astype(float)
        worst = max(worst, _ratio(diff, bound))
        assert np.all(diff <= bound), (axis, _ratio(diff, bound))
    record(f"magnetic_field {shape} complex={is_complex}: max |diff| / bound = {worst:.3f} (bound 12 eps)")


# ---------------------------------------------------------------- k_volume_average ---
def _beyond(grid, shape, left, right, stretch=1.03):
    """A grid of ``shape`` cells whose extent is that of ``grid`` moved out by the fractions ``left`` / ``right`` of it
    (negative: moved in), per axis; widths stretched away from the centre -- no node of it is a node of ``grid``."""
    h, origin = [], []
    for nodes, n, l, r in zip(_nodes(grid), shape, left, right):
        L = nodes[-1] - nodes[0]
        w = stretch ** np.abs(np.arange(n) - (n - 1) / 2.3)
        h.append(w / w.sum() * L * (1 + l + r))
        origin.append(nodes[0] - l * L)
    return emg3d.TensorMesh(h, origin)


VA_SETUPS = {
    # the output reaches beyond the input on both sides of every axis; 130 > 2 x 64 output cells along x, 9 along y
    'finer-beyond': lambda: (_stretched(67, 5, 9), _beyond(_stretched(67, 5, 9), (130, 9, 3), (.03, .05, .1), (.04, .02, .07))),
    # 130 INPUT cells along x (the adjoint's output: three blocks), 65 output cells; beyond on the right only
    'coarser': lambda: (_stretched(130, 9, 2), _beyond(_stretched(130, 9, 2), (65, 4, 1), (-.02, -.1, .05), (.03, .04, -.1))),
    'same': lambda: (_stretched(67, 5, 9), _stretched(67, 5, 9)),
}


@functools.lru_cache(maxsize=None)
def _va(name):
    """One set-up, once: grids, plan, overlap matrices, terms per output / input cell, values."""
    grid, new = VA_SETUPS[name]()
    plan = models._VolumeAverage(grid, new)
    O = overlaps(grid, new)
    k_out = np.einsum('a,b,c->abc', *[(o > 0).sum(1) for o in O])          # terms of an output cell
    k_in = np.einsum('a,b,c->abc', *[(o > 0).sum(0) for o in O])           # terms of an input cell (adjoint)
    rng = np.random.default_rng(len(name))
    v = 10 ** rng.uniform(-1, 2, grid.shape_cells)
    return dict(grid=grid, new=new, plan=plan, O=O, k_out=k_out, k_in=k_in, v=v, rng=rng, vol=_volumes(new))


def _va_forward(d, v, mode):
    """``emg3d_dev_volume_average`` with the plan's tables: fenced input, NaN output with a guard."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    plan = d['plan']
    V, vo = _fence(v.ravel('F'))
    out, oo = _guarded([int(np.prod(plan.shape_out))], torch.float64, float('nan'))
    (sx, wx, ix), (sy, wy, iy), (sz, wz, iz) = plan.tabs
    _lib.check(_lib.lib().emg3d_dev_volume_average(
        _ptr(V, vo[0]), *plan.shape_in, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(wx), _ptr(wy), _ptr(wz), _ptr(ix), _ptr(iy),
        _ptr(iz), _ptr(plan.vol), *plan.shape_out, _ptr(out, oo[0]), mode, _stream()), 'emg3d_dev_volume_average')
    torch.cuda.synchronize()
    return _split(out, oo, [plan.shape_out])[0]


def _va_linear_bound(d, v):
    """(K + 8) u sum |overlap| |v| / V per output cell with K terms: a segment length is a difference of nodes (1 u);
    wz wy (1), times wx (1), times v (1): 6 u per term; K - 1 additions; the division (1) by a volume that is a
    product of three widths (2)."""
    mag = np.einsum('ai,bj,ck,ijk->abc', *d['O'], np.abs(v).astype(LD)) / d['vol']
    return ((d['k_out'] + 8) * U * mag).astype(float)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(VA_SETUPS))
def test_volume_average_linear_vs_numpy(name):
    """Linear mode, values of either sign, entry by entry within the bound of ``_va_linear_bound``; the same grid
    returns the values (K = 1) as far as the nodes give the widths back."""
    d = _va(name)
    v = d['v'] * np.where(np.random.default_rng(5).random(d['v'].shape) < 0.5, -1.0, 1.0)
    got = _va_forward(d, v, 0)
    want = volume_average_numpy(d['grid'], d['new'], v, False)
    diff, bound = np.abs(got - want).astype(float), _va_linear_bound(d, v)
    assert np.all(np.isfinite(got)) and np.all(bound > 0)
    record(f"volume_average linear {name} {d['grid'].shape_cells} -> {d['new'].shape_cells}: max |diff| / bound = "
           f"{_ratio(diff, bound):.3f} (bound (K + 8) u, K <= {int(d['k_out'].max())})")
    assert np.all(diff <= bound)
    if name == 'same':
        # the overlap of a cell with itself is a difference of two nodes, its volume a product of widths: node k is
        # origin + cumsum(h), k + 1 roundings of at most u max |node| each, twice that on the difference
        nodes_u = sum(2 * (n.size + 1) * np.abs(n).max() / h.min() for n, h in zip(_nodes(d['grid']), d['grid'].h))
        assert np.all(d['k_out'] == 1) and np.all(np.abs(got - v) <= (9 + nodes_u) * U * np.abs(v))


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(VA_SETUPS))
def test_volume_average_log10_vs_numpy(name):
    """log10 mode: the exponent a = sum overlap log10(v) / V carries (K + 14) u sum |overlap| |log10 v| / V =: delta
    (as the linear mode, plus 3 ulp = 6 u of the device's log10 per term), and 10 ** (a + delta) = 10 ** a (1 +
    expm1(ln 10 delta)); the device's pow adds 16 ulp = 16 eps: |got - want| <= want ((1 + expm1(ln 10 delta)) (1 + 16
    eps) - 1)."""
    d = _va(name)
    v = d['v']
    got = _va_forward(d, v, 1)
    want = volume_average_numpy(d['grid'], d['new'], v, True)
    delta = (d['k_out'] + 14) * U * np.einsum('ai,bj,ck,ijk->abc', *d['O'], np.abs(np.log10(v.astype(LD)))) / d['vol']
    bound = (want * ((1 + np.expm1(np.log(LD(10)) * delta)) * (1 + 16 * EPS) - 1)).astype(float)
    diff = np.abs(got - want).astype(float)
    assert np.all(np.isfinite(got)) and np.all(bound > 0)
    record(f"volume_average log10 {name} {d['grid'].shape_cells} -> {d['new'].shape_cells}: max |diff| / bound = "
           f"{_ratio(diff, bound):.3f} (bound (K + 14) u on the exponent, pow 16 ulp)")
    assert np.all(diff <= bound)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(VA_SETUPS))
def test_volume_average_adjoint_vs_numpy(name):
    """``adjoint_add``: start + O^T (b / V) entry by entry, onto a non-zero start, and <P a, b> = <a, P^T b>.

    Entry bound: (K' + 10) u sum |overlap| |b| / V + u |start| for an input cell with K' terms: wz wy wx as above (5 u),
    b / V (1, and 2 of V), their product (1): 9 u per term, K' - 1 additions, and the final addition onto the start (1 u
    of |start| + sum). The two inner products are formed in longdouble from what the device returned, so they differ
    by at most sum |b| bound(P a) + sum |a| bound(P^T b)."""
    import torch
    d = _va(name)
    plan, rng = d['plan'], np.random.default_rng(11)
    a = rng.standard_normal(plan.shape_in)
    b = rng.standard_normal(plan.shape_out)
    start = rng.standard_normal(plan.shape_in)
    O = d['O']
    pt = np.einsum('ai,bj,ck,abc->ijk', *O, b.astype(LD) / d['vol'])
    mag = np.einsum('ai,bj,ck,abc->ijk', *O, np.abs(b).astype(LD) / d['vol'])
    res = {}
    for tag, s0 in (('start', start), ('zero', np.zeros(plan.shape_in))):
        oval, oo = _guarded([a.size], torch.float64, 0.0)
        oval[:a.size] = _up(s0.ravel('F'))
        B, bo = _fence(b.ravel('F'))
        plan.adjoint_add(B[bo[0]:bo[0] + b.size], oval[:a.size])
        torch.cuda.synchronize()
        got = _split(oval, oo, [plan.shape_in])[0]
        bound = ((d['k_in'] + 10) * U * mag + U * np.abs(s0)).astype(float)
        diff = np.abs(got - (s0 + pt)).astype(float)
        record(f"volume_average adjoint {name} onto {tag}: max |diff| / bound = {_ratio(diff, bound):.3f} "
               f"(bound (K' + 10) u, K' <= {int(d['k_in'].max())})")
        assert np.all(np.isfinite(got)) and np.all(diff <= bound)
        res[tag] = (got, bound)
    assert np.any(d['k_in'] > 0) and np.all(res['zero'][0][d['k_in'] == 0] == 0)     # cells no output cell touches
    pa = _va_forward(d, a, 0)
    lhs = np.sum(pa.astype(LD) * b)
    rhs = np.sum(a * res['zero'][0].astype(LD))
    bound = float(np.sum(np.abs(b) * _va_linear_bound(d, a)) + np.sum(np.abs(a) * res['zero'][1]))
    record(f"volume_average <P a, b> - <a, P^T b> {name}: |diff| / bound = {abs(float(lhs - rhs)) / bound:.3f}; "
           f"relative {abs(float(lhs - rhs)) / abs(float(lhs)):.2e}")
    assert abs(float(lhs - rhs)) <= bound


# ------------------------------------------------------------------ k_volume_model ---
CASES = {'isotropic': (), 'HTI': ('property_y',), 'VTI': ('property_z',), 'triaxial': ('property_y', 'property_z')}
FROM_RHO = {'Resistivity': lambda r: r, 'Conductivity': lambda r: 1 / r, 'LgResistivity': np.log10,
            'LgConductivity': lambda r: -np.log10(r), 'LnResistivity': np.log, 'LnConductivity': lambda r: -np.log(r)}
# roundings (u) of conductivity = backward(property) on the device: none, a division, pow (16 ulp), exp (3 ulp)
MAP_U = {'Conductivity': 0, 'Resistivity': 1, 'LgConductivity': 32, 'LgResistivity': 32, 'LnConductivity': 6,
         'LnResistivity': 6}


@pytest.mark.gpu
@pytest.mark.parametrize('mapping', list(FROM_RHO))
@pytest.mark.parametrize('shape', [(65, 5, 2), (130, 9, 3)])
def test_volume_model_kernel_vs_formula(shape, mapping):
    """``VolumeModel.device_arrays`` (``emg3d_dev_volume_model``) for the four anisotropy cases, with and without
    ``mu_r`` / ``epsilon_r``, at one frequency and one Laplace value, against eta = -s mu0 V (sigma + s eps0 eps_r),
    zeta = V / mu_r in longdouble.

    Bound on |eta - want|: (12 + m) u |s mu0| V (|sigma| + |s eps0 eps_r|), m = ``MAP_U[mapping]``. Count in u: V = hx
    hy hz (2); s mu0 = 2 pi f mu0 in doubles (2); times V (1); s eps0 (2), times eps_r (1); the sum (1); the complex
    product (sqrt(5) < 3); m for sigma. On |zeta - want|: 3 u V / mu_r (V: 2, the division: 1)."""
    import torch
    nx, ny, nz = shape
    grid = _stretched(*shape)
    rng = np.random.default_rng(nx + len(mapping))
    props = {n: FROM_RHO[mapping](10 ** rng.uniform(-1, 2, shape)) for n in ('property_x', 'property_y', 'property_z')}
    extras = dict(mu_r=rng.uniform(0.7, 3.0, shape), epsilon_r=rng.uniform(1., 80., shape))
    vol = _volumes(grid)
    worst_eta = worst_zeta = 0.0
    for case, names in CASES.items():
        for with_extras in (False, True):
            kw = {n: props[n] for n in ('property_x',) + names}
            model = emg3d.Model(grid, mapping=mapping, **kw, **(extras if with_extras else {}))
            assert model.case == case
            for freq in (2e6, -3e6):
                sfield = emg3d.Field(grid, frequency=freq)
                ex, ey, ez, zeta = emg3d.models.VolumeModel(model, sfield).device_arrays(_dev())
                torch.cuda.synchronize()
                assert (ey is ex) == ('property_y' not in names) and (ez is ex) == ('property_z' not in names)
                s = s_value(freq)
                smu0 = s * LD(MU_0)
                seps = s * LD(EPSILON_0) * extras['epsilon_r'].astype(LD) if with_extras else 0 * s
                for t, n in ((ex, 'property_x'), (ey, 'property_y'), (ez, 'property_z')):
                    if n != 'property_x' and n not in names:
                        continue
                    got = t.cpu().numpy().reshape(shape, order='F')
                    assert got.dtype == (np.complex128 if freq > 0 else np.float64)
                    sigma = conductivity_numpy(props[n], mapping)
                    want = -smu0 * vol * (sigma + seps)
                    bound = ((12 + MAP_U[mapping]) * U * np.abs(smu0) * vol * (np.abs(sigma) + np.abs(seps))).astype(float)
                    diff = np.abs(got - want).astype(float)
                    worst_eta = max(worst_eta, _ratio(diff, bound))
                    assert np.all(np.isfinite(got)) and np.all(diff <= bound), (case, with_extras, freq, n)
                gz = zeta.cpu().numpy().reshape(shape, order='F')
                wz = vol / extras['mu_r'].astype(LD) if with_extras else vol
                dz, bz = np.abs(gz - wz).astype(float), (3 * U * wz).astype(float)
                worst_zeta = max(worst_zeta, _ratio(dz, bz))
                assert gz.dtype == np.float64 and np.all(dz <= bz), (case, with_extras, freq)
    record(f"volume_model {shape} {mapping}: max |diff| / bound = {worst_eta:.3f} (eta, bound (12 + {MAP_U[mapping]}) "
           f"u), {worst_zeta:.3f} (zeta, bound 3 u)")


# --------------------------------------------------------------- k_source_segments ---
SRC_SHAPE = (70, 9, 5)


def _wire(kind, nseg):
    """Points of a wire inside the (70, 9, 5) grid, away from its boundary: 'walk' -- a random walk along x from
    cell 2 to cell 68 (two blocks of x-edges), y and z anywhere in the inner box; 'loop' -- a closed, tilted polygon."""
    grid = _stretched(*SRC_SHAPE)
    rng = np.random.default_rng(nseg)
    lo = np.array([n[1] for n in _nodes(grid)]) + 1.0
    hi = np.array([n[-2] for n in _nodes(grid)]) - 1.0
    if kind == 'walk':
        steps = rng.uniform(-0.3, 1.0, nseg)
        x = np.r_[0., np.cumsum(steps)]
        x = lo[0] + (x - x.min()) / (x.max() - x.min()) * (hi[0] - lo[0])
        pts = np.stack([x, rng.uniform(lo[1], hi[1], nseg + 1), rng.uniform(lo[2], hi[2], nseg + 1)], axis=1)
    else:
        phi = 2 * np.pi * np.arange(nseg) / nseg
        r = rng.uniform(0.6, 1.0, nseg)
        mid, half = (lo + hi) / 2, (hi - lo) / 2
        pts = mid + np.stack([r * np.cos(phi), r * np.sin(phi), 0.7 * r * np.cos(phi + 0.4)], axis=1) * half
        pts = np.concatenate([pts, pts[:1]])
    return grid, np.round(pts, 9)


WIRES = [('walk', 64), ('walk', 65), ('walk', 150), ('loop', 129)]
STRENGTHS = [(1.3, 2.5 - 0.5j), (1.3, 1.0), (-2.0, -1.5)]          # (frequency, strength)


@pytest.mark.gpu
@pytest.mark.parametrize('freq, strength', STRENGTHS)
@pytest.mark.parametrize('kind, nseg', WIRES)
def test_source_field_kernel_vs_host_and_conservation(kind, nseg, freq, strength):
    """``emg3d_dev_source_field`` for wires of 64, 65 and 150 segments and a closed polygon of 129 on a (70, 9, 5)
    grid: (a) against the host ``get_source_field`` (pinned to the reference by test_host_api.py; it cuts the segments
    by another method), the suite's 1e-13 relative in the 2-norm; (b) the sum of all deposits of direction a equals
    scale (p_last - p_first)[a] -- 0 for the closed loop -- whatever the pieces are.

    Bound of (b): eps N scale sum_segments |d_a| with N = 4 pieces deposits. The four weights of a piece add up to one
    in exact arithmetic and the lengths (t1 - t0) of a segment's pieces telescope, so what remains per deposit is the
    rounding of d_a, of (t1 - t0) d_a, of 1 - r and of three products, <= 7 u; every atomic add rounds once (u of the
    edge's running sum, at most N adds into one edge): (N + 7) u <= N eps times the sum of the |pieces|. Two calls
    need not agree bit for bit (the order of the atomic adds is free); nothing here asks for it."""
    import torch
    from emg3d_amd._device import _ptr, _stream
    grid, pts = _wire(kind, nseg)
    assert pts.shape == (nseg + 1, 3) and (kind == 'loop') == bool(np.array_equal(pts[0], pts[-1]))
    nx, ny, nz = grid.shape_cells
    for a, n in enumerate(_nodes(grid)):
        assert np.all(pts[:, a] > n[1]) and np.all(pts[:, a] < n[-2])
    is_complex = freq > 0
    smu0 = 2j * np.pi * freq * MU_0 if is_complex else -freq * MU_0
    scale = complex(strength) * -complex(smu0)
    sizes = [grid.n_edges_x, grid.n_edges_y, grid.n_edges_z]
    eshapes = (grid.shape_edges_x, grid.shape_edges_y, grid.shape_edges_z)
    G, go = _fence(*_nodes(grid), *grid.h, pts.ravel())
    out, oo = _guarded(sizes, torch.complex128 if is_complex else torch.float64, 0.0)
    _lib.check(_lib.lib().emg3d_dev_source_field(
        nx, ny, nz, int(is_complex), *[_ptr(G, o) for o in go], nseg + 1, scale.real, scale.imag,
        _ptr(out, oo[0]), _ptr(out, oo[1]), _ptr(out, oo[2]), _stream()), 'emg3d_dev_source_field')
    torch.cuda.synchronize()
    got = _split(out, oo, eshapes)
    assert all(np.all(np.isfinite(c)) for c in got)
    # (a)
    host = emg3d.get_source_field(grid, pts, freq, strength=strength)
    flat = np.concatenate([c.ravel('F') for c in got])
    rel = float(np.linalg.norm(flat - host.field) / np.linalg.norm(host.field))
    assert flat.dtype == host.field.dtype and np.array_equal(host._segments[0], pts)
    # (b)
    d = np.diff(pts, axis=0)
    pieces = np.ones(nseg, dtype=int)
    for a, n in enumerate(_nodes(grid)):
        lo, hi = np.minimum(pts[:-1, a], pts[1:, a]), np.maximum(pts[:-1, a], pts[1:, a])
        pieces += ((n[None, :] > lo[:, None]) & (n[None, :] < hi[:, None])).sum(1)
    ratios = []
    for a in range(3):
        total = np.sum(got[a].astype(CLD if is_complex else LD))
        want = (CLD(scale) if is_complex else LD(scale.real)) * (LD(pts[-1, a]) - LD(pts[0, a]))
        n_dep = 4 * int(pieces[d[:, a] != 0].sum())
        bound = EPS * n_dep * abs(scale) * float(np.sum(np.abs(d[:, a])))
        ratios.append(abs(complex(total - want)) / bound)
        assert np.any(got[a] != 0) and bound > 0
    record(f"source_field {kind} {nseg} segments ({int(pieces.sum())} pieces) f={freq} strength={strength}: vs host "
           f"{rel:.2e} (1e-13); |sum of deposits - scale (p_last - p_first)| / bound = "
           f"{ratios[0]:.1e} {ratios[1]:.1e} {ratios[2]:.1e} (bound N eps)")
    assert rel < 1e-13
    assert max(ratios) <= 1.0


# -------------------------------------------------------------------- k_linear_eval ---
LINEAR_SHAPES = [(66, 2, 3), (5, 70, 2), (96, 70, 50)]


@functools.lru_cache(maxsize=None)
def _linear_data(shape):
    """Axes (ascending, not uniform), values (complex N(0, 1); the real part serves the real case) and 500 points: the
    last node of every axis first, the first node second; 150 on nodes, 50 outside along one axis, the rest inside,
    shuffled."""
    rng = np.random.default_rng(sum(shape))
    axes = [np.cumsum(rng.uniform(0.5, 2.0, n)) for n in shape]
    v = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    n = 500
    xi = np.stack([rng.uniform(g[0], g[-1], n) for g in axes], axis=1)
    xi[0], xi[1] = [g[-1] for g in axes], [g[0] for g in axes]
    for a, g in enumerate(axes):                 # on nodes: 50 in all three directions, 50 in x and y, 50 in y and z
        rows = slice(2, 152) if a == 1 else slice(2, 102) if a == 0 else np.r_[2:52, 102:152]
        xi[rows, a] = g[rng.integers(0, g.size, 150 if a == 1 else 100)]
    out = np.arange(152, 202)
    xi[out, out % 3] = np.where(out % 2, -1.0, 1e3)          # below every first node / beyond every last one
    xi[2:] = xi[2:][rng.permutation(n - 2)]                  # every prefix holds all kinds
    return axes, v, xi


@pytest.mark.gpu
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('npts', [1, 64, 65, 500])
@pytest.mark.parametrize('shape', LINEAR_SHAPES)
def test_linear_eval_kernel_vs_scipy(shape, npts, is_complex):
    """``emg3d_dev_linear_eval`` called directly -- cell index and weight per axis as ``np.searchsorted`` gives them,
    index -1 for a point outside -- against ``RegularGridInterpolator(method='linear', bounds_error=False,
    fill_value=nan)``: identical NaN masks, 1e-12 absolute. The values have a NaN behind them: the upper corner of the
    last cell is the last element."""
    import torch
    from scipy.interpolate import RegularGridInterpolator
    from emg3d_amd._device import _ptr, _stream
    axes, v, xi = _linear_data(shape)
    v = v if is_complex else v.real.copy()
    xi = xi[:npts]
    idx, w = np.empty((3, npts), dtype=np.int32), np.empty((3, npts))
    for a, g in enumerate(axes):
        i = np.clip(np.searchsorted(g, xi[:, a]) - 1, 0, g.size - 2)
        w[a] = (xi[:, a] - g[i]) / (g[i + 1] - g[i])
        idx[a] = np.where((xi[:, a] >= g[0]) & (xi[:, a] <= g[-1]), i, -1)
    V, vo = _fence(v.ravel('F'))
    W, wo = _fence(w)
    out, oo = _guarded([npts], V.dtype, 0.25)
    _lib.check(_lib.lib().emg3d_dev_linear_eval(_ptr(V, vo[0]), *shape, int(is_complex), _ptr(_up(idx)), _ptr(W, wo[0]),
                                                npts, _ptr(out, oo[0]), _stream()), 'emg3d_dev_linear_eval')
    torch.cuda.synchronize()
    got = _split(out, oo, [(npts,)])[0]
    want = RegularGridInterpolator(tuple(axes), v, method='linear', bounds_error=False, fill_value=np.nan)(xi)
    m = np.isnan(want)
    assert np.array_equal(m, np.any(idx < 0, axis=0)) and not m[0]
    assert npts < 500 or m.sum() == 50
    assert np.array_equal(m, np.isnan(got)) and not np.any(got[~m] == 0.25)
    worst = float(np.abs(got[~m] - want[~m]).max())
    record(f"linear_eval {shape} {npts} points complex={is_complex}: max |diff| = {worst:.2e} (1e-12)")
    assert worst < 1e-12


# ------------------------------------------------ k_spline_filter, k_spline_eval ---
SPLINE_SHAPES = [(2, 3, 65), (66, 2, 3), (3, 130, 2), (1, 5, 70)]


@pytest.mark.gpu
@pytest.mark.parametrize('is_complex', [True, False])
@pytest.mark.parametrize('shape', SPLINE_SHAPES)
def test_spline_kernels_vs_scipy(shape, is_complex):
    """``emg3d_dev_spline_filter`` against ``ndimage.spline_filter(order=3, mode='mirror')`` and ``_spline_eval`` of
    its coefficients against ``map_coordinates(order=3, mode='constant', cval=nan)`` of the values: axes of 1, 2 and 3
    samples, passes of 6 to 390 lines. 200 coordinates from uniform(-0.5, n - 0.5) per axis, the eight corners, and 50
    more that are 0 along every axis of one sample (there, 0 is the only coordinate inside). Identical NaN masks,
    1e-12 absolute."""
    import torch
    import scipy.ndimage as ndi
    from emg3d_amd._device import _ptr, _stream
    rng = np.random.default_rng(sum(shape) + is_complex)
    v = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if is_complex else 0)
    coords = np.array([rng.uniform(-0.5, n - 0.5, 258) for n in shape])
    coords[:, 200:208] = np.array([[i * (shape[0] - 1), j * (shape[1] - 1), k * (shape[2] - 1)]
                                   for i in (0, 1) for j in (0, 1) for k in (0, 1)]).T
    for a, n in enumerate(shape):
        if n == 1:
            coords[a, 208:] = 0.0
    npts = coords.shape[1]
    parts = (lambda f, x: f(x.real) + 1j * f(x.imag)) if is_complex else (lambda f, x: f(x))
    want_coef = parts(lambda x: ndi.spline_filter(x, order=3, mode='mirror'), v)
    want = parts(lambda x: ndi.map_coordinates(x, coords, order=3, mode='constant', cval=np.nan), v)
    D, do = _guarded([v.size], torch.complex128 if is_complex else torch.float64, 0.0)
    D[:v.size] = _up(v.ravel('F'))
    C, co = _fence(coords)
    out, oo = _guarded([npts], D.dtype, 0.25)
    L = _lib.lib()
    _lib.check(L.emg3d_dev_spline_filter(_ptr(D), *shape, int(is_complex), _stream()), 'emg3d_dev_spline_filter')
    torch.cuda.synchronize()
    coef = _split(D, do, [shape])[0]
    worst_c = float(np.abs(coef - want_coef).max())
    assert worst_c < 1e-12
    _lib.check(L.emg3d_dev_spline_eval(_ptr(D), *shape, int(is_complex), _ptr(C, co[0]), npts, _ptr(out, oo[0]),
                                       _stream()), 'emg3d_dev_spline_eval')
    torch.cuda.synchronize()
    got = _split(out, oo, [(npts,)])[0]
    m = np.isnan(want)
    inside = np.all((coords >= 0) & (coords <= np.array(shape)[:, None] - 1), axis=0)
    assert np.array_equal(m, ~inside)                                 # the reference alone: NaN exactly outside
    assert np.array_equal(m, np.isnan(got)) and not np.any(got[~m] == 0.25)
    assert not m[200:208].any() and 0 < m.sum() < npts
    if min(shape) >= 2:
        assert 0 < m[:200].sum() < 200
    worst = float(np.abs(got[~m] - want[~m]).max())
    record(f"spline {shape} complex={is_complex}: coefficients max |diff| = {worst_c:.2e}, values ({int((~m).sum())} "
           f"inside) {worst:.2e} (1e-12)")
    assert worst < 1e-12


# ------------------------------------------------------------------------ method level ---
def _component_axes(grid, shape):
    return [n if shape[a] == n.size else (n[1:] + n[:-1]) / 2 for a, n in enumerate(_nodes(grid))]


def _receiver_scipy(field, rec, method):
    """Per component: the values at the receivers by SciPy (cubic: B-spline in index space, the index of a coordinate
    from the cubic interpolation of the indices over the component's own points), times the direction cosines; NaN in
    the outermost cells. Returns the responses and the tolerance 1e-12 sum |cosine| std(component)."""
    import scipy.ndimage as ndi
    from scipy.interpolate import RegularGridInterpolator, interp1d
    from scipy.special import cosdg, sindg
    grid = field.grid
    xi = np.stack(rec[:3], axis=1)
    cosines = [cosdg(rec[3]) * cosdg(rec[4]), sindg(rec[3]) * cosdg(rec[4]), sindg(rec[4])]
    resp, tol = np.zeros(xi.shape[0], dtype=field.field.dtype), np.zeros(xi.shape[0])
    for c, comp in enumerate((field.fx, field.fy, field.fz)):
        axes = _component_axes(grid, comp.shape)
        if method == 'linear':
            val = RegularGridInterpolator(tuple(axes), comp, method='linear', bounds_error=False, fill_value=np.nan)(xi)
        else:
            coords = np.array([interp1d(g, np.arange(g.size), kind='cubic', bounds_error=False,
                                        fill_value='extrapolate')(xi[:, a]) for a, g in enumerate(axes)])
            ev = lambda x: ndi.map_coordinates(x, coords, order=3, mode='constant', cval=np.nan)        # noqa: E731
            val = ev(comp.real) + 1j * ev(comp.imag) if np.iscomplexobj(comp) else ev(comp)
        resp = resp + cosines[c] * val
        tol += 1e-12 * np.abs(cosines[c]) * np.std(comp)
    outer = np.zeros(xi.shape[0], dtype=bool)
    for a, n in enumerate(_nodes(grid)):
        outer |= (xi[:, a] < n[1]) | (xi[:, a] > n[-2])
    resp[outer] = np.nan
    return resp, tol


@pytest.mark.gpu
@pytest.mark.parametrize('freq', [1.2, -2.0])
def test_get_receiver_of_both_fields_vs_scipy(freq):
    """``Field.get_receiver`` and ``get_magnetic_field(...).get_receiver`` at 150 receivers (three blocks of points)
    on a (66, 6, 5) grid, cubic and linear, against ``_receiver_scipy`` of the same field values: identical NaN masks
    (ten receivers lie in the outermost cells or outside), the suite's 1e-12 for N(0, 1) data scaled by the standard
    deviation of the component (the magnetic field of an N(0, 1) electric field is of the order 1 / (|s| mu0 h))."""
    grid = _stretched(66, 6, 5)
    rng = np.random.default_rng(31)
    nrec = 150
    lo, hi = [n[1] for n in _nodes(grid)], [n[-2] for n in _nodes(grid)]
    rec = [rng.uniform(l, h, nrec) for l, h in zip(lo, hi)] + [rng.uniform(-180, 180, nrec), rng.uniform(-90, 90, nrec)]
    rec[0][:5] = grid.nodes_x[[1, 5, 64, 65, 30]]                     # on nodes, the last admissible one among them
    rec[1][:5] = grid.nodes_y[[1, 5, 2, 5, 3]]
    rec[2][:5] = grid.nodes_z[[1, 4, 2, 4, 3]]
    rec[3][5:8], rec[4][5:8] = [0., 90., 17.], [0., 0., 90.]          # along x, y, z: components are skipped
    for k in range(10):                                                # outermost cells (even k) and outside (odd)
        a, n = k % 3, _nodes(grid)[k % 3]
        rec[a][10 + k] = [0.5 * (n[0] + n[1]), n[-1] + 3.0, 0.5 * (n[-1] + n[-2]), n[0] - 2.0][k % 4]
    rec = tuple(rec)
    dtype = complex if freq > 0 else float
    n = grid.n_edges
    efield = emg3d.Field(grid, data=(rng.standard_normal(n) + (1j * rng.standard_normal(n) if freq > 0 else 0)
                                     ).astype(dtype), frequency=freq)
    model = emg3d.Model(grid, property_x=1.0, mu_r=rng.uniform(0.7, 3.0, grid.shape_cells))
    hfield = emg3d.get_magnetic_field(model, efield)
    for kind, fld in (('e', efield), ('h', hfield)):
        for method in ('cubic', 'linear'):
            got = fld.get_receiver(rec, method=method)
            want, tol = _receiver_scipy(fld, rec, method)
            m = np.isnan(want)
            assert got.shape == want.shape and got.dtype == want.dtype and m.sum() == 10
            assert np.array_equal(m, np.isnan(got)), (kind, method)
            ratio = float(np.max(np.abs(got[~m] - want[~m]) / tol[~m]))
            record(f"get_receiver {kind} {method} f={freq}, 150 receivers: max |diff| / (1e-12 sum |cos| std) = {ratio:.3f}")
            assert ratio <= 1.0, (kind, method)


@pytest.mark.gpu
@pytest.mark.parametrize('mapping', ['Resistivity', 'LgConductivity'])
def test_interpolate_to_grid_vs_numpy(mapping):
    """``Model.interpolate_to_grid`` from (67, 5, 9) to (130, 9, 3), the mapping's default rule (log10 scale unless the
    mapping is logarithmic already, for every property array) against ``volume_average_numpy`` with the bounds of the
    two kernel tests."""
    d = _va('finer-beyond')
    grid, new = d['grid'], d['new']
    log = not mapping.startswith('L')
    rng = np.random.default_rng(41)
    rho = {n: 10 ** rng.uniform(-1, 2, grid.shape_cells) for n in ('property_x', 'property_z')}
    props = {n: FROM_RHO[mapping](r) for n, r in rho.items()}
    props.update(mu_r=rng.uniform(0.7, 3.0, grid.shape_cells), epsilon_r=rng.uniform(1., 80., grid.shape_cells))
    out = emg3d.Model(grid, mapping=mapping, **props).interpolate_to_grid(new)
    assert out.grid == new and out.mapping == mapping and out.case == 'VTI' and out.property_y is None
    worst = 0.0
    for n, v in props.items():
        got = getattr(out, n)
        want = volume_average_numpy(grid, new, v, log)
        if log:
            delta = (d['k_out'] + 14) * U * np.einsum('ai,bj,ck,ijk->abc', *d['O'], np.abs(np.log10(v.astype(LD)))) / d['vol']
            bound = (want * ((1 + np.expm1(np.log(LD(10)) * delta)) * (1 + 16 * EPS) - 1)).astype(float)
        else:
            bound = _va_linear_bound(d, v)
        diff = np.abs(got - want).astype(float)
        worst = max(worst, _ratio(diff, bound))
        assert got.shape == new.shape_cells and np.all(diff <= bound), n
    record(f"interpolate_to_grid {mapping} (67, 5, 9) -> (130, 9, 3), log={log}: max |diff| / bound = {worst:.3f}")


def test_every_kernel_runs_past_one_block():
    """What the cases above promise, per kernel: more than one block along every blocked dimension (64 along x, 4 along
    y; 64 segments, points or lines), and the sizes right at and next to a block."""
    xs, ys = {s[0] for s in EDGE}, {s[1] for s in EDGE}
    assert {1, 63, 64, 65} <= xs and max(xs) > 128 and {1, 3, 4, 5} <= ys and max(ys) > 8      # k_edge_curl
    assert any(s[2] == 1 for s in EDGE)
    for name in ('finer-beyond', 'coarser'):                          # k_volume_average: output, and adjoint output
        grid, new = VA_SETUPS[name]()
        assert max(grid.shape_cells[0], new.shape_cells[0]) > 128 and min(grid.shape_cells[0], new.shape_cells[0]) > 64
        assert new.shape_cells[1] >= 4 and grid.shape_cells[1] > 4
        for a, b in zip(_nodes(grid), _nodes(new)):
            assert not np.intersect1d(a, b).size                       # not nested
    grid, new = VA_SETUPS['finer-beyond']()
    assert all(b[0] < a[0] and b[-1] > a[-1] for a, b in zip(_nodes(grid), _nodes(new)))
    assert {s for _, s in WIRES} >= {64, 65, 150} and SRC_SHAPE[0] > 64                          # k_source_segments
    grid, pts = _wire('walk', 150)
    ix = np.searchsorted(grid.nodes_x, pts[:, 0]) - 1
    assert ix.min() < 64 <= ix.max()
    assert any(s[0] > 64 for s in LINEAR_SHAPES) and any(s[1] > 64 for s in LINEAR_SHAPES)       # k_linear_eval
    lines = [n0 * n1 * n2 // n for n0, n1, n2 in SPLINE_SHAPES for n in (n0, n1, n2) if n > 1]   # k_spline_filter
    assert min(lines) < 64 < max(lines) and {1, 2, 3} <= {n for s in SPLINE_SHAPES for n in s}
