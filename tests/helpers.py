"""Shared helpers of the test-suite (own code; no reference code)."""
import numpy as np


def relerr(a, b):
    a = np.asarray(a).ravel()
    b = np.asarray(b).ravel()
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb > 0 else 1.0))


def widths(ncore, npad, width, factor):
    """Stretched cell widths: npad growing cells, ncore constant, npad growing."""
    pad = width * np.abs(factor) ** (np.arange(npad) + 1.0)
    return np.r_[pad[::-1], np.full(ncore, float(width)), pad]


def pec_views(f):
    """The twelve views of the tangential edges on the PEC faces of a field (object with F-order fx / fy / fz)."""
    return (f.fx[:, 0, :], f.fx[:, -1, :], f.fx[:, :, 0], f.fx[:, :, -1], f.fy[0], f.fy[-1],
            f.fy[:, :, 0], f.fy[:, :, -1], f.fz[0], f.fz[-1], f.fz[:, 0], f.fz[:, -1])


def zero_pec(f):
    for v in pec_views(f):
        v[...] = 0
    return f


def pec_mask(grid):
    """Boolean vector over a field [fx|fy|fz] of `grid`: True on the tangential edges of the PEC faces."""
    from oracle import mg_ref
    m = mg_ref.Field(grid, dtype=bool)
    for v in pec_views(m):
        v[...] = True
    return m.field


def random_field(grid, dtype, rng, pec=False):
    """Random oracle field, non-zero everywhere (the boundary edges too) unless pec."""
    from oracle import mg_ref
    f = mg_ref.Field(grid, dtype=dtype)
    f.field[:] = rng.standard_normal(f.field.size)
    if dtype is complex:
        f.field[:] += 1j * rng.standard_normal(f.field.size)
    return zero_pec(f) if pec else f


def random_level(shape, case, dtype, seed, extras=False, stretch=1.1):
    """Oracle grid and volume model for kernel-against-oracle tests: random widths stretched away from the centre,
    random conductivities per anisotropy case ('isotropic' / 'VTI' / 'HTI' / 'triaxial': eta_y / eta_z alias eta_x
    where the case says so), complex (frequency domain) or real (Laplace domain: negative frequency) arithmetic.
    extras: with epsilon_r and mu_r at a frequency where the displacement term matters -- eta gets a real part of
    the size of its imaginary one, zeta = V / mu_r is not the volume. Returns (grid, vmodel, rng)."""
    from oracle import mg_ref
    rng = np.random.default_rng(seed)
    h = [rng.uniform(5., 15., n) * stretch ** np.abs(np.arange(n) - n // 2) for n in shape]
    grid = mg_ref.Grid(h, (0., 0., 0.))
    sx = 10 ** rng.uniform(-1, 1, shape)
    sy = 10 ** rng.uniform(-1, 1, shape) if case in ('HTI', 'triaxial') else None
    sz = 10 ** rng.uniform(-1, 1, shape) if case in ('VTI', 'triaxial') else None
    freq, kw = 0.7, {}
    if extras:
        freq = 2e6
        kw = dict(mu_r=rng.uniform(0.7, 3.0, shape), epsilon_r=rng.uniform(1., 80., shape))
    vm = mg_ref.volume_model(grid, freq if dtype is complex else -freq, sx, sy, sz, **kw)
    assert vm.case == case
    return grid, vm, rng


def sc_factors(sc_dir):
    """Coarsening factor (1 or 2) per direction of semicoarsening code sc_dir (reference emg3d/solver.py:891-897)."""
    return (1 if sc_dir in (1, 5, 6) else 2, 1 if sc_dir in (2, 4, 6) else 2, 1 if sc_dir in (3, 4, 5) else 2)


def admissible_sc_dirs(shape):
    """The semicoarsening codes 0..6 that coarsen only directions with an even cell count."""
    return [sc for sc in range(7) if all(f == 1 or n % 2 == 0 for f, n in zip(sc_factors(sc), shape))]


def coarse_grid(grid, sc_dir):
    from oracle import mg_ref
    rx, ry, rz = sc_factors(sc_dir)
    return mg_ref.Grid([np.diff(grid.nodes_x[::rx]), np.diff(grid.nodes_y[::ry]), np.diff(grid.nodes_z[::rz])],
                       grid.origin)


def usable_cores(cap=16):
    """Threads worth using here: the affinity mask capped by the container's CPU quota (cgroup v2) and `cap`."""
    import os
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        with open('/sys/fs/cgroup/cpu.max') as f:
            q, per = f.read().split()
            if q != 'max':
                n = min(n, max(1, int(float(q) / float(per))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, cap))
