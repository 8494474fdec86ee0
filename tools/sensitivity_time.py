"""Wall time of a Gauss-Newton inner iteration -- one ``jvec`` + one ``jtvec`` over K sources x 1 frequency of a bench
workload -- on one GPU, four ways: forward fields recomputed by every call (``keep=False``: the cost structure of
``misfit_and_gradient``), kept in HBM (``keep='device'``), kept with the K right-hand sides solved together
(``keep='device', batch=K``), and solve-free from kept source and receiver fields (``ReciprocalSensitivity``, row
``reciprocal``: ``keep='device'``, receiver solves batched by K) with its set-up cost and the number of inner iterations
after which it has paid for itself. Then the two reductions of the solve-free products alone at the run's sizes
(HIP events, median of ``--launches`` launches), beside a device-to-device copy of the same byte count and the torch
composition of the same result, interleaved. Writes profiles/sensitivity_times.txt. Last leg: the diagonal of the
Gauss-Newton Hessian, ``ReciprocalSensitivity.hessian_diagonal`` (one pass over the kept fields), against the row-by-row
route through the existing ``jtvec`` -- 2 ns nr calls, squared and added --, taking turns, and its kernel alone beside a
copy of its byte count. Writes profiles/hessian_diagonal_times.txt. Leg ``gram``: the data-space normal matrix,
``ReciprocalSensitivity.data_gram``, against the route through the existing ``jtvec`` -- 2 N calls on unit data and 1j
times them, stacked, then ``(Jhat * m) @ Jhat.T`` in NumPy --, taking turns, with one frequency and with two; its kernel
alone beside a copy of its byte count, and the achieved FMA rate. Writes profiles/data_gram_times.txt.
``--field-dtype single`` runs the reciprocal, hessian and gram legs on fields kept in single precision.
Leg ``single``: ``field_dtype='double'`` and ``'single'`` side by side, taking turns in every measurement -- kept bytes,
the inner iteration, ``hessian_diagonal`` and ``data_gram``, the four kernels alone (HIP events) with the two reductions in
TB/s on the bytes their stacks hold, and the differences of the five products. Writes
profiles/reciprocal_single_times.txt.
Leg ``block``: K vectors per pass over the kept fields, K = 1, 2, 4, 8, 16, for ``field_dtype='double'``
and ``'single'`` -- the two block kernels alone against K launches of the single-vector kernels (HIP events, taking turns in an order drawn anew for every round;
TB/s on the bytes the stacks hold plus the w / t rows), then ``hessian_vec_block`` on a device block, result left on the
device, against K calls of ``hessian_vec`` on NumPy vectors, with ``keep='device'`` and ``keep='host'``. Writes
profiles/block_products_times.txt.
Leg ``gnsolve``: one iteration of the block PCG of ``ReciprocalSensitivity.gauss_newton_solve``, K = 1, 4,
8 dampings, for ``field_dtype='double'`` and ``'single'``: the new kernels alone (HIP events) with their rates on
algorithmic bytes beside a device copy that moves the same bytes, then 10 iterations split by events into the Hessian pass
and every new kernel, and the same 10 iterations written with torch operations around ``hessian_vec_block`` and a slicing
regulariser -- what a user can write without the method --, the two taking turns for five rounds. Writes
profiles/gauss_newton_solve_times.txt. Then, for 'double', the weighted / sparse-norm regulariser: its
kernel with weights only, norms of 1 and general norms beside the plain kernel and a copy of its bytes, and an iteration of
``gauss_newton_solve`` weighted against plain. Writes profiles/weighted_regulariser_times.txt.
Leg ``gndata``: the data-space (Woodbury) preconditioner of ``gauss_newton_solve`` beside Jacobi, K = 1, 4,
8: the application pass beside the Hessian pass, its vector kernels and the filter beside a copy of their bytes, an
iteration of either route, the set-up by its steps, and iterations and wall time to ``tol = 1e-3`` at three dampings, the
two routes taking turns for five rounds. Writes profiles/data_preconditioner_times.txt.
Leg ``blocks``: the cell blocks of the Hessian and block-Jacobi on the workload's VTI model: the kernel
``emg3d_dev_hessian_cell_blocks`` beside ``emg3d_dev_hessian_diagonal`` on the same inputs, taking turns (HIP events), an
iteration of ``gauss_newton_solve`` with ``'block'`` beside ``True``, and iterations and wall time to ``tol = 1e-3`` of
``True``, ``'block'`` and ``'data'`` at the three dampings of the ``gndata`` leg. Writes profiles/hessian_blocks_times.txt.
Leg ``svd``: the randomised truncated SVD: ``emg3d_dev_block_gram`` and ``emg3d_dev_block_rotate`` alone at
8, 24 and 56 columns beside a copy of their bytes, an orthonormalisation beside the same steps from torch operations, and
``sensitivity_svd`` at rank 16 and 48 beside ``data_gram`` + ``eigh`` + one ``jtvec_block``, taking turns. Writes
profiles/sensitivity_svd_times.txt.

    python tools/sensitivity_time.py [--workload marine128] [--sources 4] [--repeat 3] [--launches 30]
                                     [--leg all|products|hessian|gram|single|block|gnsolve|gndata|blocks|svd]
                                     [--field-dtype double|single]
                                     [--out profiles/sensitivity_times.txt]
                                     [--hessian-out profiles/hessian_diagonal_times.txt]
                                     [--gram-out profiles/data_gram_times.txt]
                                     [--single-out profiles/reciprocal_single_times.txt]
                                     [--block-out profiles/block_products_times.txt]
                                     [--gnsolve-out profiles/gauss_newton_solve_times.txt]
                                     [--weighted-out profiles/weighted_regulariser_times.txt]
                                     [--gndata-out profiles/data_preconditioner_times.txt]
                                     [--blocks-out profiles/hessian_blocks_times.txt]
                                     [--svd-out profiles/sensitivity_svd_times.txt]

(COMMIT=<hash> in the environment names the commit on a box without git.)
"""
import argparse
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import torch                              # noqa: E402
import emg3d_amd as emg3d                 # noqa: E402
from emg3d_amd import gradient            # noqa: E402
from bench import csrc_sha16, workload    # noqa: E402


def commit():
    if os.environ.get('COMMIT'):
        return os.environ['COMMIT']
    try:
        return subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], text=True,
                                       stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return 'unknown'


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def timed(fn, count):
    """Median, fastest and spread of ``count`` launches (ms, HIP events), after two warm-up launches."""
    ms = []
    for i in range(count + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= 2:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms) - min(ms))


def wall(fn):
    """(wall time of ``fn()`` in ms, synchronised; its result)."""
    t0 = sync()
    out = fn()
    return 1e3 * (sync() - t0), out


def kernel_block(rec, say, launches):
    """``emg3d_dev_sensitivity_dots`` and ``emg3d_dev_sensitivity_combine`` alone on the kept fields of ``rec``."""
    from emg3d_amd import _lib
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    (E, X), = rec._stacks.values()
    ns, nr, n = len(E), len(X), E.shape[1]
    sp, el = gradient.ReciprocalSensitivity._sp(E), E.element_size()
    dev = E.device
    gen = torch.Generator(device=dev).manual_seed(0)
    w = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    C = torch.randn(ns, nr, dtype=torch.complex128, device=dev, generator=gen)
    ws_len = L.emg3d_sensitivity_dots_ws_len(ns, nr, n)
    ws = torch.empty(ws_len, dtype=torch.float64, device=dev)
    out = torch.empty(ns * nr, dtype=torch.complex128, device=dev)
    t = torch.empty(n, dtype=torch.complex128, device=dev)
    bytes_dots = (ns + nr) * el * n + 8 * n                  # every field and w read once
    bytes_comb = (ns + nr) * el * n + 16 * n                 # every field read once, t written
    src = {b: torch.empty(b // 2, dtype=torch.uint8, device=dev) for b in (bytes_dots, bytes_comb)}
    dst = {b: torch.empty_like(a) for b, a in src.items()}

    def k_dots():
        _lib.check(getattr(L, 'emg3d_dev_sensitivity_dots' + sp)(n, 1, _ptr(E), E.stride(0), ns, _ptr(X), X.stride(0), nr,
                                                                 _ptr(w), 0.5, -1.5, _ptr(out), _ptr(ws), ws_len, _stream()),
                   'emg3d_dev_sensitivity_dots' + sp)

    def k_comb():
        _lib.check(getattr(L, 'emg3d_dev_sensitivity_combine' + sp)(n, 1, _ptr(E), E.stride(0), ns, _ptr(X), X.stride(0), nr,
                                                                    _ptr(C), _ptr(t), _stream()),
                   'emg3d_dev_sensitivity_combine' + sp)
    what = [('dots: kernel', k_dots, bytes_dots),
            ('dots: torch (E * w) @ X.T', lambda: (Ew * w) @ Xw.T * (0.5 - 1.5j), bytes_dots),
            ('dots: copy', lambda: dst[bytes_dots].copy_(src[bytes_dots]), bytes_dots),
            ('combine: kernel', k_comb, bytes_comb),
            ('combine: torch ((C @ X) * E).sum(0)', lambda: ((C @ Xw) * Ew).sum(0), bytes_comb),
            ('combine: copy', lambda: dst[bytes_comb].copy_(src[bytes_comb]), bytes_comb)]
    Ew, Xw = (E, X) if not sp else (E.to(torch.complex128), X.to(torch.complex128))    # (torch: from fp64 copies)
    ref_d, ref_c = (Ew * w) @ Xw.T * (0.5 - 1.5j), ((C @ Xw) * Ew).sum(0)
    k_dots()
    k_comb()
    say(f"kernels alone: n {n:,} edges, ns {ns}, nr {nr}, {E.dtype}; algorithmic bytes dots {bytes_dots:,} = (ns + nr) {el} n + "
        f"8 n, combine {bytes_comb:,} = (ns + nr) {el} n + 16 n; a copy reads half of that count and writes the other half; "
        f"kernel vs torch, max-norm relative: dots {float((out.view(ns, nr) - ref_d).abs().max() / ref_d.abs().max()):.1e}, "
        f"combine {float((t - ref_c).abs().max() / ref_c.abs().max()):.1e}")
    del ref_d, ref_c
    ms = {name: [] for name, _, _ in what}
    for rep in range(launches + 3):                  # three warm-up rounds; the candidates take turns
        for name, fn, _ in what:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= 3:
                ms[name].append(a.elapsed_time(b))
    for name, _, nbytes in what:
        q = np.percentile(ms[name], [50, 25, 75, 0, 100])
        say(f"  {name:38s} median {q[0]:8.4f} ms (quartiles {q[1]:.4f} .. {q[2]:.4f}, range {q[3]:.4f} .. {q[4]:.4f}; "
            f"{len(ms[name])} launches, HIP events) = {nbytes / q[0] / 1e9:7.3f} TB/s on algorithmic bytes")


def hessian_block(rec, say, repeat, launches):
    """``hessian_diagonal`` against 2 ns nr calls of ``jtvec`` (unit datum and 1j times it per source, receiver and
    frequency; squared and added), all weights one; then ``emg3d_dev_hessian_diagonal`` alone on the kept fields."""
    from emg3d_amd import _lib
    from emg3d_amd._device import _ptr, _stream
    nrec = len(rec._rec[0])

    def row_by_row():
        out, calls = 0.0, 0
        for pair in rec.pairs:
            for r in range(nrec):
                unit = np.zeros(nrec, dtype=complex)
                unit[r] = 1.0
                for y in (unit, 1j * unit):
                    out = out + rec.jtvec({pair: y}) ** 2
                    calls += 1
        return out, calls
    times = {'one pass': [], 'row by row': []}
    for r in range(repeat + 1):                     # run 0: warm-up; the two routes take turns
        n0 = dict(rec.n_solves)
        t0 = sync()
        H = rec.hessian_diagonal()
        t1 = sync()
        R, calls = row_by_row()
        t2 = sync()
        say(f"run {r}{' (warm-up)' if r == 0 else '':10s}: hessian_diagonal {1e3 * (t1 - t0):9.3f} ms   row by row ({calls} jtvec) "
            f"{1e3 * (t2 - t1):9.3f} ms   ratio {(t2 - t1) / (t1 - t0):7.1f}   solves { {k: rec.n_solves[k] - n0[k] for k in n0} }"
            f"   max |H - rows| / max H {float(np.max(np.abs(H - R)) / np.max(H)):.2e}   |H| {np.linalg.norm(H):.6e}")
        if r:
            times['one pass'].append(t1 - t0)
            times['row by row'].append(t2 - t1)
    one, rows = (float(np.mean(times[k])) for k in ('one pass', 'row by row'))
    say(f"mean of {repeat}: hessian_diagonal {1e3 * one:.3f} ms, row by row {1e3 * rows:.3f} ms: ratio {rows / one:.1f} "
        f"(fastest runs {1e3 * min(times['one pass']):.3f} ms, {1e3 * min(times['row by row']):.3f} ms: "
        f"{min(times['row by row']) / min(times['one pass']):.1f})")
    del H, R
    # the kernel alone
    L = _lib.lib()
    (E, X), = rec._stacks.values()
    ns, nr, n = len(E), len(X), E.shape[1]
    grid = rec.model.grid
    nx, ny, nz = grid.shape_cells
    ncell = grid.n_cells
    rows3 = gradient._EXPAND[rec.model.case]
    nrows = max(rows3) + 1
    dev = E.device
    vol = rec._computational(rec.pairs[0])[3]
    w = torch.ones(ns * nr, dtype=torch.float64, device=dev)
    h = torch.zeros(nrows * ncell, dtype=torch.float64, device=dev)
    sp, el = gradient.ReciprocalSensitivity._sp(E), E.element_size()
    nbytes = (ns + nr) * el * n + 8 * ncell + 16 * nrows * ncell        # every field once, volumes, h read and written
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def kernel():
        _lib.check(getattr(L, 'emg3d_dev_hessian_diagonal' + sp)(nx, ny, nz, 1, _ptr(E), E.stride(0), ns, _ptr(X), X.stride(0),
                                                                 nr, _ptr(w), *rows3, 1.0, _ptr(vol), _ptr(h), ncell, _stream()),
                   'emg3d_dev_hessian_diagonal' + sp)
    what = [('hessian_diagonal: kernel', kernel), ('hessian_diagonal: copy', lambda: dst.copy_(src))]
    ms = {name: [] for name, _ in what}
    for rep in range(launches + 3):                  # three warm-up rounds; the candidates take turns
        for name, fn in what:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= 3:
                ms[name].append(a.elapsed_time(b))
    say(f"kernel alone: {nx} x {ny} x {nz} cells, n {n:,} edges, ns {ns}, nr {nr}, {E.dtype}, rows {rows3}; algorithmic bytes "
        f"{nbytes:,} = (ns + nr) {el} n + 8 n_cells + 16 rows n_cells; fp64 FMA ~ 55 ns nr n_cells = {55 * ns * nr * ncell:,}; a copy "
        "reads half of that count and writes the other half")
    for name, _ in what:
        q = np.percentile(ms[name], [50, 25, 75, 0, 100])
        say(f"  {name:28s} median {q[0]:8.4f} ms (quartiles {q[1]:.4f} .. {q[2]:.4f}, range {q[3]:.4f} .. {q[4]:.4f}; "
            f"{len(ms[name])} launches, HIP events) = {nbytes / q[0] / 1e9:7.3f} TB/s on algorithmic bytes")


def gram_block(rec, say, repeat, launches, kernel):
    """``data_gram`` against 2 N calls of ``jtvec`` (unit datum and 1j times it per pair and receiver), stacked, and
    ``(Jhat * m) @ Jhat.T`` on the host, all model weights one; with ``kernel``: ``emg3d_dev_data_gram`` alone on the
    kept fields of the (one) frequency."""
    from emg3d_amd import _lib
    from emg3d_amd._device import _ptr, _stream
    nrec, npairs = len(rec._rec[0]), len(rec.pairs)
    N = npairs * nrec

    def route():
        Jhat, calls = None, 0
        for k, pair in enumerate(rec.pairs):
            for r in range(nrec):
                unit = np.zeros(nrec, dtype=complex)
                unit[r] = 1.0
                for half, y in enumerate((unit, 1j * unit)):
                    row = rec.jtvec({pair: y}).ravel()
                    if Jhat is None:
                        Jhat = np.empty((2 * N, row.size))
                    Jhat[half * N + k * nrec + r] = row
                    calls += 1
        t = sync()
        return Jhat @ Jhat.T, calls, t                   # (m = 1)
    times = {'data_gram': [], 'route': [], 'calls': []}
    for r in range(repeat + 1):                     # run 0: warm-up; the two routes take turns
        n0 = dict(rec.n_solves)
        t0 = sync()
        G = rec.data_gram()
        t1 = sync()
        R, calls, tj = route()
        t2 = sync()
        say(f"run {r}{' (warm-up)' if r == 0 else '':10s}: data_gram {1e3 * (t1 - t0):9.3f} ms   route ({calls} jtvec + product) "
            f"{1e3 * (t2 - t1):9.3f} ms (jtvec calls {1e3 * (tj - t1):9.3f} ms)   ratio {(t2 - t1) / (t1 - t0):7.1f}   solves "
            f"{ {k: rec.n_solves[k] - n0[k] for k in n0} }   max |G - route| / max G {float(np.max(np.abs(G - R)) / np.max(G)):.2e}"
            f"   symmetric {bool(np.array_equal(G, G.T))}   |G| {np.linalg.norm(G):.6e}")
        if r:
            times['data_gram'].append(t1 - t0)
            times['route'].append(t2 - t1)
            times['calls'].append(tj - t1)
    one, rows, calls_only = (float(np.mean(times[k])) for k in ('data_gram', 'route', 'calls'))
    say(f"mean of {repeat}: data_gram {1e3 * one:.3f} ms, route {1e3 * rows:.3f} ms (its jtvec calls alone {1e3 * calls_only:.3f} "
        f"ms): ratio {rows / one:.1f} (fastest runs {1e3 * min(times['data_gram']):.3f} ms, {1e3 * min(times['route']):.3f} ms: "
        f"{min(times['route']) / min(times['data_gram']):.1f})")
    del G, R
    if not kernel:
        return
    L = _lib.lib()
    (E, X), = rec._stacks.values()
    ns, nr, n = len(E), len(X), E.shape[1]
    grid = rec.model.grid
    nx, ny, nz = grid.shape_cells
    ncell = grid.n_cells
    rows3 = gradient._EXPAND[rec.model.case]
    nrows = max(rows3) + 1
    dev = E.device
    vol = rec._computational(rec.pairs[0])[3]
    mw = torch.ones(nrows * ncell, dtype=torch.float64, device=dev)
    M = 2 * ns * nr
    out = torch.empty(M * M, dtype=torch.float64, device=dev)
    ws_len = L.emg3d_data_gram_ws_len(nx, ny, nz, 1, ns * nr, ns * nr)
    ws = torch.empty(ws_len, dtype=torch.float64, device=dev)
    sp, el = gradient.ReciprocalSensitivity._sp(E), E.element_size()
    nbytes = (ns + nr) * el * n + 8 * ncell + 8 * nrows * ncell + 16 * ws_len   # fields, volumes, weights; ws written and read
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def kernel_call():
        _lib.check(getattr(L, 'emg3d_dev_data_gram' + sp)(
            nx, ny, nz, 1, _ptr(E), E.stride(0), ns, _ptr(X), X.stride(0), nr, 0.0, 1e-5, _ptr(E), E.stride(0), ns, _ptr(X),
            X.stride(0), nr, 0.0, 1e-5, *rows3, _ptr(mw), ncell, _ptr(vol), _ptr(out), M, _ptr(ws), ws_len, _stream()),
            'emg3d_dev_data_gram' + sp)
    what = [('data_gram: kernel (two launches)', kernel_call), ('data_gram: copy', lambda: dst.copy_(src))]
    ms = {name: [] for name, _ in what}
    for rep in range(launches + 3):                  # three warm-up rounds; the candidates take turns
        for name, fn in what:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= 3:
                ms[name].append(a.elapsed_time(b))
    # rows: 4 edges x 4 FMA per complex product and pair and direction (3 directions in all) + the scaling;
    # update: the full M x M tile per cell and property row (the kernel does not skip the lower triangle)
    fma_rows, fma_full, fma_tri = 55 * ns * nr * ncell, M * M * nrows * ncell, M * (M + 1) // 2 * nrows * ncell
    say(f"kernel alone: {nx} x {ny} x {nz} cells, n {n:,} edges, ns {ns}, nr {nr}, {E.dtype}, rows {rows3}, M {M}; algorithmic "
        f"bytes {nbytes:,} = (ns + nr) {el} n + 8 n_cells + 8 rows n_cells + 16 ws_len; fp64 FMA: rows of J ~ 55 ns nr n_cells = "
        f"{fma_rows:,}, update as issued M^2 rows n_cells = {fma_full:,} (one triangle: {fma_tri:,}); a copy reads half of the "
        "byte count and writes the other half")
    for name, _ in what:
        q = np.percentile(ms[name], [50, 25, 75, 0, 100])
        say(f"  {name:34s} median {q[0]:8.4f} ms (quartiles {q[1]:.4f} .. {q[2]:.4f}, range {q[3]:.4f} .. {q[4]:.4f}; "
            f"{len(ms[name])} launches, HIP events) = {nbytes / q[0] / 1e9:7.3f} TB/s on algorithmic bytes")
    med = float(np.median(ms[what[0][0]]))
    say(f"  FMA rate of the kernel: issued {(fma_rows + fma_full) / med / 1e9:.2f} T FMA/s = {2 * (fma_rows + fma_full) / med / 1e9:.2f} "
        f"TFLOP/s fp64; on the count with one triangle {(fma_rows + fma_tri) / med / 1e9:.2f} T FMA/s = "
        f"{2 * (fma_rows + fma_tri) / med / 1e9:.2f} TFLOP/s")


def single_block(recs, say, repeat, launches, v, y):
    """``recs``: {'double': ..., 'single': ...} after ``forward()``, one frequency. Every measurement lets the two take
    turns, 'double' first, so that a busy spell of the box hits both."""
    from emg3d_amd import _lib
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    names = list(recs)
    for name, rec in recs.items():
        (E, X), = rec._stacks.values()
        say(f"{name:7s} kept_bytes {rec.kept_bytes:,} B ({len(E) + len(X)} fields of {E.shape[1]:,} edges, {E.dtype}, row stride "
            f"{E.stride(0):,} elements = {E.stride(0) * E.element_size():,} B)")
    # ---- the methods: inner iteration, hessian_diagonal, data_gram
    res = {name: {} for name in names}
    methods = (('jvec', lambda r: r.jvec(v)), ('jtvec', lambda r: r.jtvec(y)), ('hessian_diagonal', lambda r: r.hessian_diagonal()),
               ('data_gram', lambda r: r.data_gram()))
    times = {(name, m): [] for name in names for m, _ in methods}
    for r in range(repeat + 1):                       # run 0: warm-up
        for name in names:
            line = f"{name:7s} run {r}{' (warm-up)' if r == 0 else '':10s}:"
            for m, fn in methods:
                t0 = sync()
                res[name][m] = fn(recs[name])
                t1 = sync()
                line += f"  {m} {1e3 * (t1 - t0):8.3f}"
                if r:
                    times[(name, m)].append(t1 - t0)
            say(line + " ms")
    for name in names:
        t = {m: np.array(times[(name, m)]) for m, _ in methods}
        it = t['jvec'] + t['jtvec']
        say(f"mean of {repeat}: {name:7s} inner iteration (jvec + jtvec) {1e3 * it.mean():.3f} ms (fastest {1e3 * it.min():.3f}, "
            f"slowest {1e3 * it.max():.3f}); hessian_diagonal {1e3 * t['hessian_diagonal'].mean():.3f} ms (fastest "
            f"{1e3 * t['hessian_diagonal'].min():.3f}); data_gram {1e3 * t['data_gram'].mean():.3f} ms (fastest "
            f"{1e3 * t['data_gram'].min():.3f}); synchronised, results on the host")
    # ---- the five products: single against double
    w1 = {p: np.ones(len(y[p])) for p in y}
    res['double']['hessian_vec'], res['single']['hessian_vec'] = (recs[k].hessian_vec(v, w1) for k in ('double', 'single'))

    def rel(a, b):
        if isinstance(a, dict):
            a, b = np.concatenate([a[k] for k in a]), np.concatenate([b[k] for k in b])
        return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    say("single against double, max-norm relative difference: " + ", ".join(
        f"{m} {rel(res['single'][m], res['double'][m]):.2e}" for m in ('jvec', 'jtvec', 'hessian_diagonal', 'hessian_vec', 'data_gram')))
    # ---- the four kernels alone
    what = []
    keep = []                                            # (the buffers of the closures)
    for name, rec in recs.items():
        (E, X), = rec._stacks.values()
        ns, nr, n = len(E), len(X), E.shape[1]
        sp, el = rec._sp(E), E.element_size()
        dev = E.device
        grid = rec.model.grid
        nx, ny, nz = grid.shape_cells
        ncell = grid.n_cells
        rows3 = gradient._EXPAND[rec.model.case]
        nrows = max(rows3) + 1
        vol = rec._computational(rec.pairs[0])[3]
        gen = torch.Generator(device=dev).manual_seed(0)
        w = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
        C = torch.randn(ns, nr, dtype=torch.complex128, device=dev, generator=gen)
        ws_len = L.emg3d_sensitivity_dots_ws_len(ns, nr, n)
        ws = torch.empty(ws_len, dtype=torch.float64, device=dev)
        out = torch.empty(ns * nr, dtype=torch.complex128, device=dev)
        t = torch.empty(n, dtype=torch.complex128, device=dev)
        wt = torch.ones(ns * nr, dtype=torch.float64, device=dev)
        h = torch.zeros(nrows * ncell, dtype=torch.float64, device=dev)
        mw = torch.ones(nrows * ncell, dtype=torch.float64, device=dev)
        M = 2 * ns * nr
        gout = torch.empty(M * M, dtype=torch.float64, device=dev)
        gws_len = L.emg3d_data_gram_ws_len(nx, ny, nz, 1, ns * nr, ns * nr)
        gws = torch.empty(gws_len, dtype=torch.float64, device=dev)
        keep.append((w, C, ws, out, t, wt, h, mw, gout, gws))
        stacks = (ns + nr) * el * n

        def k_dots(E=E, X=X, n=n, ns=ns, nr=nr, w=w, out=out, ws=ws, ws_len=ws_len, sp=sp):
            _lib.check(getattr(L, 'emg3d_dev_sensitivity_dots' + sp)(n, 1, _ptr(E), E.stride(0), ns, _ptr(X), X.stride(0), nr,
                                                                     _ptr(w), 0.5, -1.5, _ptr(out), _ptr(ws), ws_len, _stream()),
                       'emg3d_dev_sensitivity_dots' + sp)

        def k_comb(E=E, X=X, n=n, ns=ns, nr=nr, C=C, t=t, sp=sp):
            _lib.check(getattr(L, 'emg3d_dev_sensitivity_combine' + sp)(n, 1, _ptr(E), E.stride(0), ns, _ptr(X), X.stride(0), nr,
                                                                        _ptr(C), _ptr(t), _stream()),
                       'emg3d_dev_sensitivity_combine' + sp)

        def k_hess(E=E, X=X, ns=ns, nr=nr, wt=wt, h=h, sp=sp):
            _lib.check(getattr(L, 'emg3d_dev_hessian_diagonal' + sp)(nx, ny, nz, 1, _ptr(E), E.stride(0), ns, _ptr(X),
                                                                     X.stride(0), nr, _ptr(wt), *rows3, 1.0, _ptr(vol), _ptr(h),
                                                                     ncell, _stream()), 'emg3d_dev_hessian_diagonal' + sp)

        def k_gram(E=E, X=X, ns=ns, nr=nr, mw=mw, gout=gout, M=M, gws=gws, gws_len=gws_len, sp=sp):
            _lib.check(getattr(L, 'emg3d_dev_data_gram' + sp)(
                nx, ny, nz, 1, _ptr(E), E.stride(0), ns, _ptr(X), X.stride(0), nr, 0.0, 1e-5, _ptr(E), E.stride(0), ns, _ptr(X),
                X.stride(0), nr, 0.0, 1e-5, *rows3, _ptr(mw), ncell, _ptr(vol), _ptr(gout), M, _ptr(gws), gws_len, _stream()),
                'emg3d_dev_data_gram' + sp)
        what += [(f'dots {name}', k_dots, stacks), (f'combine {name}', k_comb, stacks), (f'hessian_diagonal {name}', k_hess, stacks),
                 (f'data_gram {name}', k_gram, stacks)]
    order = [q for kernel in ('dots', 'combine', 'hessian_diagonal', 'data_gram') for q in what if q[0].split()[0] == kernel]
    ms = {q[0]: [] for q in order}
    for rep in range(launches + 3):                  # three warm-up rounds; double and single of a kernel take turns
        for label, fn, _ in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= 3:
                ms[label].append(a.elapsed_time(b))
    say(f"kernels alone on the kept fields (HIP events, {launches} launches each, double and single taking turns); TB/s on the "
        "bytes the stacks hold, (ns + nr) x n x 16 B or 8 B; dots reads 8 n B of weights besides, combine writes 16 n B")
    for label, _, nbytes in order:
        q = np.percentile(ms[label], [50, 25, 75, 0, 100])
        say(f"  {label:26s} median {q[0]:8.4f} ms (quartiles {q[1]:.4f} .. {q[2]:.4f}, range {q[3]:.4f} .. {q[4]:.4f}) = "
            f"{nbytes / q[0] / 1e9:7.3f} TB/s on {nbytes:,} B")
    for kernel in ('dots', 'combine', 'hessian_diagonal', 'data_gram'):
        d, s1 = (np.median(ms[f'{kernel} {k}']) for k in ('double', 'single'))
        say(f"  {kernel}: single / double = {s1 / d:.3f} (medians)")
    del keep


BLOCK_K = (1, 2, 4, 8, 16)


def block_kernels(rec, say, launches):
    """``emg3d_dev_sensitivity_dots_block`` / ``_combine_block`` with K vectors against K launches of
    ``emg3d_dev_sensitivity_dots`` / ``_combine`` on the kept fields of ``rec`` (one frequency, ``keep='device'``)."""
    from emg3d_amd import _lib
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    (E, X), = rec._stacks.values()
    ns, nr, n = len(E), len(X), E.shape[1]
    sp, el = rec._sp(E), E.element_size()
    dev = E.device
    kmax = max(BLOCK_K)
    gen = torch.Generator(device=dev).manual_seed(0)
    W = torch.randn(kmax, n, dtype=torch.float64, device=dev, generator=gen)
    C = torch.randn(kmax, ns, nr, dtype=torch.complex128, device=dev, generator=gen)
    T = torch.empty(kmax, n, dtype=torch.complex128, device=dev)
    out = torch.empty(kmax * ns * nr, dtype=torch.complex128, device=dev)
    ws_len = L.emg3d_sensitivity_dots_block_ws_len(ns, nr, kmax, n)
    ws = torch.empty(ws_len, dtype=torch.float64, device=dev)
    one_len = L.emg3d_sensitivity_dots_ws_len(ns, nr, n)
    stacks = (ns + nr) * el * n
    names = {k: 'emg3d_dev_sensitivity_' + k + sp for k in ('dots', 'combine', 'dots_block', 'combine_block')}

    def dots_block(K):
        _lib.check(getattr(L, names['dots_block'])(n, 1, _ptr(E), E.stride(0), ns, _ptr(X), X.stride(0), nr, _ptr(W), n, K, 0.5,
                                                   -1.5, _ptr(out), _ptr(ws), ws_len, _stream()), names['dots_block'])

    def dots_each(K):
        for k in range(K):
            _lib.check(getattr(L, names['dots'])(n, 1, _ptr(E), E.stride(0), ns, _ptr(X), X.stride(0), nr, _ptr(W, k * n), 0.5,
                                                 -1.5, _ptr(out, k * ns * nr), _ptr(ws), one_len, _stream()), names['dots'])

    def combine_block(K):
        _lib.check(getattr(L, names['combine_block'])(n, 1, _ptr(E), E.stride(0), ns, _ptr(X), X.stride(0), nr, _ptr(C), K,
                                                      _ptr(T), n, _stream()), names['combine_block'])

    def combine_each(K):
        for k in range(K):
            _lib.check(getattr(L, names['combine'])(n, 1, _ptr(E), E.stride(0), ns, _ptr(X), X.stride(0), nr,
                                                    _ptr(C, k * ns * nr), _ptr(T, k * n), _stream()), names['combine'])
    # the two routes give the same numbers (dots: to rounding; combine: the same bits)
    dots_block(kmax)
    a = out.clone()
    combine_block(kmax)
    b = T.clone()
    dots_each(kmax)
    combine_each(kmax)
    say(f"kernels alone: n {n:,} edges, ns {ns}, nr {nr}, {E.dtype}; K = {kmax}: dots_block vs {kmax} x dots, max-norm relative "
        f"{float((a - out).abs().max() / out.abs().max()):.1e}; combine_block vs {kmax} x combine bit-identical: "
        f"{bool(torch.equal(b, T))}. Bytes: block = stacks {stacks:,} + K rows (w: 8 n, t: 16 n); K launches = K x (stacks + one "
        f"row). fp64 FMA per edge: dots_block ns nr (4 + 2 K), K x dots 6 ns nr K (complex); HIP events around the K launches, "
        f"the candidates taking turns in an order drawn anew for every round, {launches} timed rounds after 3 warm-up rounds")
    del a, b
    for K in BLOCK_K:
        what = [(f'dots_block K={K}', lambda K=K: dots_block(K), stacks + 8 * n * K),
                (f'{K} x dots', lambda K=K: dots_each(K), K * (stacks + 8 * n)),
                (f'combine_block K={K}', lambda K=K: combine_block(K), stacks + 16 * n * K),
                (f'{K} x combine', lambda K=K: combine_each(K), K * (stacks + 16 * n))]
        ms = {name: [] for name, _, _ in what}
        shuffle = np.random.default_rng(K)           # a new order every round: neither a candidate's position nor its
        for rep in range(launches + 3):              # predecessor (whose traffic is what the caches hold) stays the same
            for name, fn, _ in [what[i] for i in shuffle.permutation(len(what))]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep >= 3:
                    ms[name].append(e0.elapsed_time(e1))
        q = {name: np.percentile(ms[name], [50, 25, 75]) for name in ms}
        for name, _, nbytes in what:
            say(f"  {name:22s} median {q[name][0]:8.4f} ms (quartiles {q[name][1]:.4f} .. {q[name][2]:.4f}) = "
                f"{nbytes / q[name][0] / 1e9:7.3f} TB/s on {nbytes:,} B")
        for blk, each, ceil in ((what[0][0], what[1][0], K * (stacks + 8 * n) / (stacks + 8 * n * K)),
                                (what[2][0], what[3][0], K * (stacks + 16 * n) / (stacks + 16 * n * K))):
            spread = max(q[blk][2] - q[blk][1], q[each][2] - q[each][1])
            say(f"  {each} / {blk}: {q[each][0] / q[blk][0]:.2f} x (medians; ceiling of the byte count {ceil:.2f} x); difference "
                f"{q[each][0] - q[blk][0]:+.4f} ms, larger quartile spread {spread:.4f} ms")


def block_methods(rec, say, repeat, label):
    """``hessian_vec_block`` on a device block, the result left on the device, against K calls of ``hessian_vec`` on NumPy
    vectors (the only route without the block methods), taking turns; all weights one."""
    grid = rec.model.grid
    ncomp = gradient._NCOMP[rec.model.case]
    rng = np.random.default_rng(1)
    for K in BLOCK_K:
        V = rng.standard_normal((K, ncomp) + tuple(grid.shape_cells))
        B = rec.to_device(V)
        tb, te = [], []
        for r in range(repeat + 1):                     # run 0: warm-up
            t0 = sync()
            H = rec.hessian_vec_block(B)
            t1 = sync()
            R = [rec.hessian_vec(v) for v in V]
            t2 = sync()
            if r:
                tb.append(t1 - t0)
                te.append(t2 - t1)
        diff = float(np.max(np.abs(rec.from_device(H) - np.stack(R))) / np.max(np.abs(np.stack(R))))
        say(f"  {label}, K = {K:2d}: hessian_vec_block (device block in and out, columns_per_pass 8) mean {1e3 * np.mean(tb):9.3f} ms "
            f"(fastest {1e3 * min(tb):9.3f}); {K} x hessian_vec (NumPy in and out) mean {1e3 * np.mean(te):9.3f} ms (fastest "
            f"{1e3 * min(te):9.3f}); ratio of the means {np.mean(te) / np.mean(tb):6.1f}; max-norm relative difference {diff:.1e}")
        del H, R, B


GN_K = (1, 4, 8)
GN_ITERATIONS, GN_ROUNDS, GN_CHECK = 10, 5, 4
GN_REG = (1e-6, 1.0, 1.0, 1.0)              # smallness, smoothness x / y / z


def gnsolve_block(rec, say, launches):
    """One iteration of the block PCG two ways on the kept fields of ``rec``: with the kernels of csrc/regularise.h in
    the order ``gauss_newton_solve`` launches them, and with torch operations around ``hessian_vec_block``."""
    from emg3d_amd._blockpass import _BlockPCG
    grid = rec.model.grid
    n, ncell = gradient._NCOMP[rec.model.case], grid.n_cells
    nx, ny, nz = grid.shape_cells
    dev = torch.device('cuda', torch.cuda.current_device())
    w = rec._check_weights(None)
    geo = rec._regulariser_geometry(None, dev)
    hx, hy, hz = geo[3:6]
    hd = rec._hessian_diagonal_block(w, dev)[0].contiguous()
    rd = rec._regulariser_diagonal(geo, GN_REG, None, dev)
    lam0 = float(hd.mean() / rd.mean())
    # the slicing regulariser of the torch route: its coefficients are made once, as a user would
    shape = (nz, ny, nx)
    hs = [h.view(v) for h, v in zip((hx, hy, hz), ((1, 1, nx), (1, ny, 1), (nz, 1, 1)))]
    vol = hs[0] * hs[1] * hs[2]
    faces = []
    for d, (dim, h) in enumerate(zip((-1, -2, -3), (hx, hy, hz))):
        area = (hs[1] * hs[2], hs[0] * hs[2], hs[0] * hs[1])[d]
        dist = (0.5 * (h[:-1] + h[1:])).view([len(h) - 1 if k == 3 + dim else 1 for k in range(3)])
        faces.append((dim, GN_REG[1 + d] * area / dist))

    def torch_R(v):
        v = v.view((v.shape[0], n) + shape)
        out = GN_REG[0] * vol * v
        for dim, coef in faces:
            m = v.shape[dim]
            d = coef * (v.narrow(dim, 0, m - 1) - v.narrow(dim, 1, m - 1))
            out.narrow(dim, 0, m - 1).add_(d)
            out.narrow(dim, 1, m - 1).sub_(d)
        return out.view(v.shape[0], n, ncell)

    rng = np.random.default_rng(2)
    for K in GN_K:
        lam = lam0 * 10.0 ** np.linspace(-1, 1, K)
        b = rec.to_device(rng.standard_normal((K, n) + tuple(grid.shape_cells)))
        ps = rec._pass(dev, K, 8, w)                       # the pass and the step pieces of gauss_newton_solve, tol 1e-30
        pcg = _BlockPCG(ps, lam, b.clone(), 1e-30, None, (hd, rd))
        host, q = pcg.table.cpu(), torch.zeros_like(b)

        def k_reg():
            rec._regulariser(geo, GN_REG, pcg.p, q, beta=1.0, lam=pcg.lam, pq=pcg.pq, ws=pcg.rws)

        def k_hessian():
            nonlocal q
            q = rec._gradient_block(ps.hessian_vec(pcg.p))

        def k_update():
            pcg.update(0, q)

        def start():
            pcg.table.copy_(host)
            pcg.x.zero_()
            pcg.r.copy_(b)
            pcg.step(1)

        def fused(parts=None):
            """GN_ITERATIONS iterations as gauss_newton_solve runs them; ``parts``: event times per piece are added."""
            start()
            for it in range(1, GN_ITERATIONS + 1):
                for name, fn in (('hessian pass', k_hessian), ('regulariser', k_reg), ('update', k_update),
                                 ('scalar step', lambda: pcg.scalar(0)), ('direction', lambda: pcg.direction(0))):
                    if parts is None:
                        fn()
                    else:
                        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        fn()
                        e.record()
                        parts.setdefault(name, []).append((a, e))
                if it % GN_CHECK == 0 or it == GN_ITERATIONS:
                    state = pcg.table.cpu().numpy()
            return pcg.x, state[:, 5] / state[:, 1]

        tl = torch.from_numpy(lam).to(dev).view(K, 1, 1)

        def composed():
            """The same iterations from torch operations: what a user writes around hessian_vec_block."""
            xt, rt = torch.zeros_like(b), b.clone()
            m = 1.0 / (hd + tl * rd)
            z = rt * m
            pt = z.clone()
            rz = (rt * z).sum((1, 2))
            bb = (rt * rt).sum((1, 2))
            for it in range(1, GN_ITERATIONS + 1):
                qt = rec.hessian_vec_block(pt) + tl * torch_R(pt)
                alpha = (rz / (pt * qt).sum((1, 2))).view(K, 1, 1)
                xt += alpha * pt
                rt -= alpha * qt
                z = rt * m
                new = (rt * z).sum((1, 2))
                rr = (rt * rt).sum((1, 2))
                pt = z + (new / rz).view(K, 1, 1) * pt
                rz = new
                if it % GN_CHECK == 0 or it == GN_ITERATIONS:
                    rel = (rr / bb).cpu().numpy()
            return xt, rel

        # the kernels alone on a running state (one iteration in, so that p and q hold what an iteration gives them)
        start(), k_hessian(), k_reg()
        elems = K * n * ncell
        shared = (n + 1) * ncell * 8
        for name, fn, nbytes in (('regulariser', k_reg, elems * 24), ('update', k_update, elems * 48 + shared),
                                 ('direction', lambda: pcg.direction(0), elems * 24 + shared)):
            src = torch.empty(nbytes // 16, dtype=torch.float64, device=dev)
            dst = torch.empty_like(src)
            med, best, _ = timed(fn, launches)
            cmed, cbest, _ = timed(lambda: dst.copy_(src), launches)
            say(f"  K = {K}: {name:12s} median {med:7.3f} ms (fastest {best:7.3f}), {nbytes / 1e6:8.1f} MB algorithmic = "
                f"{nbytes / med / 1e9:5.2f} TB/s; copy that moves the same bytes {cmed:7.3f} ms (fastest {cbest:7.3f}) = "
                f"{nbytes / cmed / 1e9:5.2f} TB/s; ratio to the copy rate {cmed / med:4.2f}")
            del src, dst
        med, best, _ = timed(lambda: pcg.scalar(0), launches)
        say(f"  K = {K}: scalar step  median {med:7.3f} ms (fastest {best:7.3f}), one workgroup")
        # ten iterations, the two routes taking turns
        fused(), composed()                                  # warm-up
        tf, tc = [], []
        for _ in range(GN_ROUNDS):
            t, (xf, relf) = wall(fused)
            tf.append(t / GN_ITERATIONS)
            t, (xc, relc) = wall(composed)
            tc.append(t / GN_ITERATIONS)
        diff = float((xf - xc).abs().max() / xc.abs().max())
        parts = {}
        fused(parts)
        torch.cuda.synchronize()
        split = ", ".join(f"{name} {np.mean([a.elapsed_time(e) for a, e in ev]):.3f}" for name, ev in parts.items())
        say(f"  K = {K}: per iteration (wall, synchronised, {GN_ITERATIONS} iterations, table read every {GN_CHECK}), rounds: "
            f"new kernels {' '.join(f'{t:.3f}' for t in tf)} ms (mean {np.mean(tf):.3f}, spread {max(tf) - min(tf):.3f}); torch "
            f"operations {' '.join(f'{t:.3f}' for t in tc)} ms (mean {np.mean(tc):.3f}, spread {max(tc) - min(tc):.3f}); ratio "
            f"of the means {np.mean(tc) / np.mean(tf):.2f}; max-norm relative difference of x {diff:.1e}; |r|^2 / |b|^2 after "
            f"{GN_ITERATIONS}: {relf.max():.2e} / {relc.max():.2e}")
        say(f"  K = {K}: split of an iteration (HIP events, mean, ms): {split}")
        t0 = time.perf_counter()
        _, info = rec.gauss_newton_solve(b, lam, smallness=GN_REG[0], smoothness=GN_REG[1:], tol=1e-30, maxit=GN_ITERATIONS,
                                        check_every=GN_CHECK)
        torch.cuda.synchronize()
        say(f"  K = {K}: gauss_newton_solve(maxit={GN_ITERATIONS}) with its set-up (hessian_diagonal, diag R, table): "
            f"{1e3 * (time.perf_counter() - t0):.1f} ms, {info['hessian_passes']} passes, states {info['state'].tolist()}")
        del b, q, pcg, ps


GN_NORMS = (('weights only', (2.0, 2.0, 2.0, 2.0)), ('norms 1', (1.0, 1.0, 1.0, 1.0)), ('norms general', (0.5, 1.5, 1.2, 0.7)))
GN_EPS = (1e-2, 1e-4)


def weighted_block(rec, say, launches):
    """The weighted / sparse-norm regulariser on the model grid of ``rec``: its kernel with weights
    only, with norms of 1 and with general norms beside the plain kernel of the same build and beside a copy of its
    bytes; then an iteration of ``gauss_newton_solve``, weighted against plain, as the difference of runs of 2 x and
    1 x ``GN_ITERATIONS`` iterations (the set-up drops out), the two taking turns."""
    from emg3d_amd import _lib
    L = _lib.lib()
    grid = rec.model.grid
    n, ncell = gradient._NCOMP[rec.model.case], grid.n_cells
    nx, ny, nz = grid.shape_cells
    dev = torch.device('cuda', torch.cuda.current_device())
    geo = rec._regulariser_geometry(None, dev)
    rng = np.random.default_rng(4)
    wd = torch.from_numpy(rng.uniform(0.2, 5.0, (n, ncell))).to(dev)
    ud = torch.from_numpy(rng.standard_normal((n, ncell))).to(dev)

    hd = rec._hessian_diagonal_block(rec._check_weights(None), dev)[0]
    lam0 = float(hd.mean()) / (GN_REG[1] * float(np.mean(grid.h[0])))
    for K in GN_K:
        lam = lam0 * 10.0 ** np.linspace(-1, 1, K)
        dlam = torch.from_numpy(lam).to(dev)
        b = rec.to_device(rng.standard_normal((K, n) + tuple(grid.shape_cells)))
        p, q = b.clone(), torch.zeros_like(b)
        pq = torch.zeros(K, dtype=torch.float64, device=dev)
        rws = torch.empty(L.emg3d_model_regulariser_ws_len(nx, ny, nz, K * n, n), dtype=torch.float64, device=dev)
        elems = K * n * ncell
        plain = timed(lambda: rec._regulariser(geo, GN_REG, p, q, beta=1.0, lam=dlam, pq=pq, ws=rws), launches)
        say(f"  K = {K}: plain kernel       median {plain[0]:7.3f} ms (fastest {plain[1]:7.3f}), {elems * 24 / 1e6:8.1f} MB algorithmic")
        for name, norms in GN_NORMS:
            sparse = any(e != 2.0 for e in norms)
            irls = (wd, norms, ud if sparse else None, GN_EPS if sparse else (0.0, 0.0))
            nbytes = elems * 24 + (2 if sparse else 1) * n * ncell * 8
            med, best, _ = timed(lambda: rec._regulariser(geo, GN_REG, p, q, beta=1.0, lam=dlam, pq=pq, ws=rws, irls=irls),
                                 launches)
            src = torch.empty(nbytes // 16, dtype=torch.float64, device=dev)
            dst = torch.empty_like(src)
            cmed, cbest, _ = timed(lambda: dst.copy_(src), launches)
            del src, dst
            say(f"  K = {K}: {name:18s} median {med:7.3f} ms (fastest {best:7.3f}), {nbytes / 1e6:8.1f} MB algorithmic = "
                f"{nbytes / med / 1e9:5.2f} TB/s; copy that moves the same bytes {cmed:7.3f} ms (fastest {cbest:7.3f}); ratio "
                f"to the copy rate {cmed / med:4.2f}; to the plain kernel {med / plain[0]:4.2f} x, + {1e3 * (med - plain[0]):.0f} us")
        kw = dict(smallness=GN_REG[0], smoothness=GN_REG[1:], tol=1e-30, check_every=GN_CHECK)
        routes = (('plain', {}), ('weighted, norms 1', dict(cell_weights=wd, norms=GN_NORMS[1][1], linearise_at=ud,
                                                           irls_eps=GN_EPS)))

        def run(extra, its):
            return wall(lambda: rec.gauss_newton_solve(b, lam, maxit=its, **kw, **extra))[0]
        for _, extra in routes:
            run(extra, GN_ITERATIONS)                          # warm-up
        per = {name: [] for name, _ in routes}
        for _ in range(GN_ROUNDS):
            for name, extra in routes:
                per[name].append((run(extra, 2 * GN_ITERATIONS) - run(extra, GN_ITERATIONS)) / GN_ITERATIONS)
        say(f"  K = {K}: gauss_newton_solve per iteration (wall, {2 * GN_ITERATIONS} minus {GN_ITERATIONS} iterations, table read "
            f"every {GN_CHECK}), rounds: " + "; ".join(
                f"{name} {' '.join(f'{t:.3f}' for t in ts)} ms (mean {np.mean(ts):.3f}, spread {max(ts) - min(ts):.3f})"
                for name, ts in per.items()) + f"; weighted / plain {np.mean(per[routes[1][0]]) / np.mean(per['plain']):.3f}")
        del b, p, q


GD_FACTORS = (1e-2, 1.0, 1e2)                # dampings of the solves to tol, times tr H / tr R
GD_MAXIT = 400


def data_preconditioner_block(rec, say, launches):
    """The data-space preconditioner beside Jacobi on the kept fields of ``rec``: the application pass
    beside the Hessian pass, the three vector kernels and the filter beside a device copy of their bytes, an iteration
    of either route as the difference of runs of 2 x and 1 x ``GN_ITERATIONS`` iterations (the set-up drops out), the
    set-up by its steps, and iterations and wall time to ``tol = 1e-3`` at three dampings -- the two routes taking turns."""
    from emg3d_amd import _lib
    from emg3d_amd._blockpass import _BlockPCG
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    grid = rec.model.grid
    n, ncell = gradient._NCOMP[rec.model.case], grid.n_cells
    dev = torch.device('cuda', torch.cuda.current_device())
    w = rec._check_weights(None)
    geo = rec._regulariser_geometry(None, dev)
    hd = rec._hessian_diagonal_block(w, dev)[0].contiguous()
    rd = rec._regulariser_diagonal(geo, GN_REG, None, dev)
    lam0 = float(hd.sum() / (n * rd.sum()))
    reg = dict(smallness=GN_REG[0], smoothness=GN_REG[1:])

    rng = np.random.default_rng(2)
    for K in GN_K:
        lam = lam0 * 10.0 ** np.linspace(-1, 1, K)
        b = rec.to_device(rng.standard_normal((K, n) + tuple(grid.shape_cells)))
        pre = rec._data_preconditioner_setup(dev, w, rd, None, None)
        M, rank = pre['n_data'], pre['rank']
        ps = rec._pass(dev, K, 8, w)                       # the pass and the step pieces of gauss_newton_solve
        pcg = _BlockPCG(ps, lam, b.clone(), 1e-30, None, pre=pre)
        table, g = pcg.table, torch.zeros_like(b)
        table[:, 2], table[:, 3] = 1.0, 2.0              # a running state: <r,z> new / old, <p,q>
        pcg.pq.fill_(1.0)
        pcg.p.copy_(b)

        def k_hessian():
            rec._gradient_block(ps.hessian_vec(pcg.p))

        def k_apply():
            rec._gradient_block(ps.precondition(pcg.u, pre, table))
        d, y = torch.randn((K, M), dtype=torch.float64, device=dev), torch.zeros((K, M), dtype=torch.float64, device=dev)
        fws_len = L.emg3d_data_space_filter_ws_len(rank, K)
        fws = torch.empty(fws_len, dtype=torch.float64, device=dev)

        def k_filter():
            _lib.check(L.emg3d_dev_data_space_filter(M, rank, K, _ptr(pre['q']), _ptr(pre['eigenvalues']), _ptr(pre['s']),
                                                     _ptr(d), _ptr(y), _ptr(table), _ptr(fws), fws_len, _stream()),
                       'emg3d_dev_data_space_filter')
        pcg.scale(0), k_hessian(), k_apply()
        for _ in range(2):                                       # the two passes taking turns
            hm, hb, hs = timed(k_hessian, launches)
            am, ab, asp = timed(k_apply, launches)
            say(f"  K = {K}: Hessian pass median {hm:7.3f} ms (fastest {hb:7.3f}, spread {hs:6.3f}); application pass median "
                f"{am:7.3f} ms (fastest {ab:7.3f}, spread {asp:6.3f}); ratio of the medians {am / hm:4.2f}")
        elems = K * n * ncell
        for name, fn, nbytes in (('scale', lambda: pcg.scale(0), elems * 16 + ncell * 8),
                                 ('finish', lambda: pcg.finish(0, g), elems * 32 + ncell * 8),
                                 ('direction_z', lambda: pcg.direction(0), elems * 24)):
            src = torch.empty(nbytes // 16, dtype=torch.float64, device=dev)
            dst = torch.empty_like(src)
            med, best, _ = timed(fn, launches)
            cmed, cbest, _ = timed(lambda: dst.copy_(src), launches)
            say(f"  K = {K}: {name:12s} median {med:7.3f} ms (fastest {best:7.3f}), {nbytes / 1e6:8.1f} MB algorithmic = "
                f"{nbytes / med / 1e9:5.2f} TB/s; copy that moves the same bytes {cmed:7.3f} ms (fastest {cbest:7.3f}); ratio to "
                f"the copy rate {cmed / med:4.2f}")
            del src, dst
        pcg.p.copy_(b)
        med, best, _ = timed(k_filter, launches)
        src = torch.empty(max(2, M * rank), dtype=torch.float64, device=dev)
        dst = torch.empty_like(src)
        cmed, cbest, _ = timed(lambda: dst.copy_(src), launches)
        say(f"  K = {K}: filter       median {med:7.3f} ms (fastest {best:7.3f}), M = {M}, rank {rank}, Q read twice = "
            f"{2 * M * rank * 8 / 1e3:.1f} kB in {2 * -(-K // 8)} launches; a copy of those bytes {cmed:7.3f} ms (fastest "
            f"{cbest:7.3f}): bound by launches, not by bytes")
        del src, dst
        say(f"  K = {K}: set-up of the preconditioner (ms): " +
            ", ".join(f"{name} {1e3 * t:.2f}" for name, t in pre['seconds'].items()) + f"; M = {M}")

        def run(route, its):
            return rec.gauss_newton_solve(b, lam, tol=1e-30, maxit=its, check_every=GN_CHECK, precondition=route, **reg)
        for route in (True, 'data'):
            run(route, 2)                                        # warm-up
        per = {True: [], 'data': []}
        for _ in range(GN_ROUNDS):
            for route in (True, 'data'):
                t1, _ = wall(lambda: run(route, GN_ITERATIONS))
                t2, (_, info) = wall(lambda: run(route, 2 * GN_ITERATIONS))
                per[route].append((t2 - t1) / GN_ITERATIONS)
        say(f"  K = {K}: per iteration (wall, (2 x {GN_ITERATIONS} - {GN_ITERATIONS}) iterations / {GN_ITERATIONS}), rounds: Jacobi "
            f"{' '.join(f'{t:.3f}' for t in per[True])} ms (mean {np.mean(per[True]):.3f}); data "
            f"{' '.join(f'{t:.3f}' for t in per['data'])} ms (mean {np.mean(per['data']):.3f}); ratio of the means "
            f"{np.mean(per['data']) / np.mean(per[True]):.2f}")
        del b, g, pcg, ps, pre
    # what users care about: iterations and wall time to tol 1e-3, one right-hand side, three dampings in one call
    lam = lam0 * np.array(GD_FACTORS)
    b = rec.to_device(rng.standard_normal((1, n) + tuple(grid.shape_cells)))[0]

    def solve(route):
        return rec.gauss_newton_solve(b, lam, tol=1e-3, maxit=GD_MAXIT, check_every=GN_CHECK, precondition=route, **reg)
    for route in (True, 'data'):
        rec.gauss_newton_solve(b, lam, tol=1e-3, maxit=2, precondition=route, **reg)
    for _ in range(GN_ROUNDS):
        for route in (True, 'data'):
            t, (_, info) = wall(lambda: solve(route))
            say(f"  to tol 1e-3, dampings {GD_FACTORS} x tr H / tr R ({lam0:.3e}), maxit {GD_MAXIT}: "
                f"{'Jacobi' if route is True else 'data  '} iterations {info['iterations'].tolist()}, states "
                f"{info['state'].tolist()}, relative residuals {[f'{v:.1e}' for v in info['relative_residual']]}, "
                f"{info['hessian_passes']} + {info['preconditioner_passes']} passes, {t:.1f} ms with the set-up")


def cell_blocks_block(rec, say, launches):
    """The cell blocks of the Hessian and block-Jacobi on the kept fields of ``rec``: the two kernels on
    the same inputs taking turns, an iteration of ``gauss_newton_solve`` with ``'block'`` beside ``True`` as the
    difference of runs of 2 x and 1 x ``GN_ITERATIONS`` iterations, and iterations and wall time to ``tol = 1e-3`` of the
    three preconditioners at the dampings of ``data_preconditioner_block``."""
    from emg3d_amd import _lib
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    (E, X), = rec._stacks.values()
    ns, nr, nedges = len(E), len(X), E.shape[1]
    grid = rec.model.grid
    nx, ny, nz = grid.shape_cells
    n, ncell = gradient._NCOMP[rec.model.case], grid.n_cells
    rows3 = gradient._EXPAND[rec.model.case]
    npack = n * (n + 1) // 2
    dev = E.device
    vol = rec._computational(rec.pairs[0])[3]
    wd = torch.ones(ns * nr, dtype=torch.float64, device=dev)
    h = torch.zeros(npack * ncell, dtype=torch.float64, device=dev)
    sp, el = gradient.ReciprocalSensitivity._sp(E), E.element_size()

    def kernel(name):
        name += sp
        fn = getattr(L, name)
        return lambda: _lib.check(fn(nx, ny, nz, 1, _ptr(E), E.stride(0), ns, _ptr(X), X.stride(0), nr, _ptr(wd), *rows3, 1.0,
                                     _ptr(vol), _ptr(h), ncell, _stream()), name)
    what = [('hessian_diagonal', kernel('emg3d_dev_hessian_diagonal'), n),
            ('hessian_cell_blocks', kernel('emg3d_dev_hessian_cell_blocks'), npack)]
    ms = {name: [] for name, _, _ in what}
    for r in range(launches + 3):                    # three warm-up rounds; the two take turns
        for name, fn, _ in what:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= 3:
                ms[name].append(a.elapsed_time(b))
    say(f"kernels alone: {nx} x {ny} x {nz} cells, {nedges:,} edges, ns {ns}, nr {nr}, {E.dtype}, rows {rows3}: both read "
        f"(ns + nr) {el} n = {(ns + nr) * el * nedges:,} B of fields; the diagonal stages every direction once per row and "
        f"tile, the blocks once per tile, and form {npack} products per pair instead of {n}")
    med = {}
    for name, _, nrows in what:
        q = np.percentile(ms[name], [50, 25, 75, 0, 100])
        med[name] = q[0]
        nbytes = (ns + nr) * el * nedges + 8 * ncell + 16 * nrows * ncell
        say(f"  {name:20s} median {q[0]:8.4f} ms (quartiles {q[1]:.4f} .. {q[2]:.4f}, range {q[3]:.4f} .. {q[4]:.4f}; "
            f"{len(ms[name])} launches, HIP events) = {nbytes / q[0] / 1e9:7.3f} TB/s on algorithmic bytes ({nrows} rows of h)")
    say(f"  ratio of the medians, cell blocks / diagonal: {med['hessian_cell_blocks'] / med['hessian_diagonal']:.2f}")
    t, B = wall(lambda: rec.hessian_cell_blocks(on_device=True))
    t, B = wall(lambda: rec.hessian_cell_blocks(on_device=True))
    corr = (B[n] / torch.sqrt(B[0] * B[1])).abs()
    corr = corr[torch.isfinite(corr)]
    say(f"method hessian_cell_blocks(on_device=True): {t:.3f} ms; |B_01| / sqrt(B_00 B_11): median "
        f"{float(corr.median()):.3f}, 90 % {float(torch.quantile(corr[::8], 0.9)):.3f}, max {float(corr.max()):.3f}")
    del B, corr

    w = rec._check_weights(None)
    geo = rec._regulariser_geometry(None, dev)
    hd = rec._hessian_diagonal_block(w, dev)[0]
    rd = rec._regulariser_diagonal(geo, GN_REG, None, dev)
    lam0 = float(hd.sum() / (n * rd.sum()))
    del hd, rd
    reg = dict(smallness=GN_REG[0], smoothness=GN_REG[1:])
    rng = np.random.default_rng(2)
    routes = ((True, 'Jacobi'), ('block', 'block '))
    for K in GN_K:
        lam = lam0 * 10.0 ** np.linspace(-1, 1, K)
        b = rec.to_device(rng.standard_normal((K, n) + tuple(grid.shape_cells)))

        def run(route, its):
            return rec.gauss_newton_solve(b, lam, tol=1e-30, maxit=its, check_every=GN_CHECK, precondition=route, **reg)
        for route, _ in routes:
            run(route, 2)                                        # warm-up
        per = {route: [] for route, _ in routes}
        for _ in range(GN_ROUNDS):
            for route, _ in routes:
                t1, _ = wall(lambda: run(route, GN_ITERATIONS))
                t2, _ = wall(lambda: run(route, 2 * GN_ITERATIONS))
                per[route].append((t2 - t1) / GN_ITERATIONS)
        say(f"  K = {K}: per iteration (wall, (2 x {GN_ITERATIONS} - {GN_ITERATIONS}) iterations / {GN_ITERATIONS}), rounds: Jacobi "
            f"{' '.join(f'{t:.3f}' for t in per[True])} ms (mean {np.mean(per[True]):.3f}); block "
            f"{' '.join(f'{t:.3f}' for t in per['block'])} ms (mean {np.mean(per['block']):.3f}); ratio of the means "
            f"{np.mean(per['block']) / np.mean(per[True]):.2f}")
        del b
    lam = lam0 * np.array(GD_FACTORS)
    b = rec.to_device(rng.standard_normal((1, n) + tuple(grid.shape_cells)))[0]
    routes += (('data', 'data  '),)

    def solve(route):
        return rec.gauss_newton_solve(b, lam, tol=1e-3, maxit=GD_MAXIT, check_every=GN_CHECK, precondition=route, **reg)
    for route, _ in routes:
        rec.gauss_newton_solve(b, lam, tol=1e-3, maxit=2, precondition=route, **reg)
    for _ in range(3):
        for route, label in routes:
            t, (_, info) = wall(lambda: solve(route))
            say(f"  to tol 1e-3, dampings {GD_FACTORS} x tr H / tr R ({lam0:.3e}), maxit {GD_MAXIT}: {label} iterations "
                f"{info['iterations'].tolist()}, states {info['state'].tolist()}, relative residuals "
                f"{[f'{v:.1e}' for v in info['relative_residual']]}, {info['hessian_passes']} + "
                f"{info['preconditioner_passes']} passes, {t:.1f} ms with the set-up")


SVD_COLS = (8, 24, 56)                   # columns of the kernels alone: l of rank 16 and 48 with oversample 8, and 8
SVD_RANKS = (16, 48)


def svd_block(rec, say, repeat, launches):
    """The randomised SVD on the kept fields of ``rec``: ``emg3d_dev_block_gram`` and
    ``emg3d_dev_block_rotate`` alone at ``SVD_COLS`` columns, each taking turns with a device copy of its bytes (HIP
    events); an orthonormalisation of a block beside the same two SVQB steps written with torch operations (``Y @ Y.T``,
    ``T.T.contiguous() @ Y``), taking turns; ``sensitivity_svd`` at ``SVD_RANKS`` beside the same factorisation by
    ``data_gram`` + ``eigh`` + one ``jtvec_block``, taking turns, and how far their singular values are apart."""
    from emg3d_amd import _lib
    from emg3d_amd._blockpass import _BlockOrth, _svqb_rotation
    from emg3d_amd._device import _ptr, _stream
    L = _lib.lib()
    grid = rec.model.grid
    ncomp, ncell = gradient._NCOMP[rec.model.case], grid.n_cells
    n = ncomp * ncell
    dev = next(iter(rec._stacks.values()))[0].device
    gen = torch.Generator(device=dev).manual_seed(0)
    say(f"kernels alone: blocks of n = {ncomp} x {ncell:,} = {n:,} doubles per column, contiguous rows; medians of {launches} "
        "launches (HIP events), every kernel taking turns with a device copy that moves its bytes")
    for ncol in SVD_COLS:
        Y = torch.randn((ncol, n), dtype=torch.float64, device=dev, generator=gen)
        out = torch.empty_like(Y)
        T = torch.randn((ncol, ncol), dtype=torch.float64, device=dev, generator=gen)
        G = torch.empty(ncol * ncol, dtype=torch.float64, device=dev)
        ws = torch.empty(L.emg3d_block_gram_ws_len(n, ncol), dtype=torch.float64, device=dev)

        def k_gram():
            _lib.check(L.emg3d_dev_block_gram(n, ncol, _ptr(Y), n, _ptr(G), _ptr(ws), _stream()), 'emg3d_dev_block_gram')

        def k_rotate():
            _lib.check(L.emg3d_dev_block_rotate(n, ncol, ncol, _ptr(Y), n, _ptr(T), _ptr(out), n, _stream()),
                       'emg3d_dev_block_rotate')
        half = Y[:max(ncol // 2, 1)]
        what = [('block_gram', k_gram, 8 * ncol * n, lambda: out[:len(half)].copy_(half), 16 * len(half) * n),
                ('block_rotate', k_rotate, 16 * ncol * n, lambda: out.copy_(Y), 16 * ncol * n)]
        for name, fn, nbytes, copy, cbytes in what:
            ms = {'kernel': [], 'copy': []}
            for r in range(launches + 3):                # three warm-up rounds; the two take turns
                for key, f in (('kernel', fn), ('copy', copy)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    f()
                    b.record()
                    b.synchronize()
                    if r >= 3:
                        ms[key].append(a.elapsed_time(b))
            q, c = np.percentile(ms['kernel'], [50, 25, 75]), np.percentile(ms['copy'], [50, 25, 75])
            flops = (ncol * (ncol + 1) if name == 'block_gram' else 2 * ncol * ncol) * n
            say(f"  {name:12s} ncol {ncol:2d}: median {q[0]:8.4f} ms (quartiles {q[1]:.4f} .. {q[2]:.4f}) = "
                f"{nbytes / q[0] / 1e9:6.3f} TB/s on {nbytes:,} algorithmic B, {flops / q[0] / 1e9:6.2f} TFLOP/s fp64; copy of "
                f"{cbytes:,} B (read + written): {c[0]:8.4f} ms (quartiles {c[1]:.4f} .. {c[2]:.4f}) = {cbytes / c[0] / 1e9:6.3f} "
                f"TB/s; kernel / copy {q[0] / c[0]:.2f}")
        del Y, out, T, G, ws, half, what
    say(f"orthonormalisation of a block (two SVQB steps; wall, synchronised, download of G, eigh on the host and upload of T "
        f"included), the library's kernels beside torch operations (Y @ Y.T, T.T.contiguous() @ Y), taking turns, {repeat} rounds after a warm-up:")
    for ncol in SVD_COLS:
        Y0 = torch.randn((ncol, n), dtype=torch.float64, device=dev, generator=gen)
        orth = _BlockOrth(dev, ncol, n)

        def by_library():
            return orth(Y0.clone())[0]

        def by_torch():
            Q = Y0
            for _ in range(2):
                T = torch.from_numpy(_svqb_rotation((Q @ Q.T).cpu().numpy())).to(dev)
                Q = T.T.contiguous() @ Q
            return Q
        per = {'library': [], 'torch': []}
        for r in range(repeat + 1):
            for key, f in (('library', by_library), ('torch', by_torch)):
                t, Q = wall(f)
                if r:
                    per[key].append(t)
        err = {key: float((f() @ f().T - torch.eye(ncol, dtype=torch.float64, device=dev)).abs().max())
               for key, f in (('library', by_library), ('torch', by_torch))}
        say(f"  ncol {ncol:2d}: library {' '.join(f'{t:.3f}' for t in per['library'])} ms (mean {np.mean(per['library']):.3f}); torch "
            f"{' '.join(f'{t:.3f}' for t in per['torch'])} ms (mean {np.mean(per['torch']):.3f}); ratio of the means torch / library "
            f"{np.mean(per['torch']) / np.mean(per['library']):.2f}; max |Q Q^T - I|: library {err['library']:.1e}, torch "
            f"{err['torch']:.1e}")
        del Y0, orth
    M = 2 * len(rec.pairs) * len(rec._rec[0])
    say(f"sensitivity_svd(rank, oversample=8, power_iterations=1, on_device=True), all weights one, M = {M}, beside data_gram + "
        f"eigh + one jtvec_block of `rank` columns (V = J^T U / s, on the device); wall, synchronised, taking turns, {repeat} "
        "rounds after a warm-up:")
    for rank in SVD_RANKS:
        def by_sketch():
            return rec.sensitivity_svd(rank, oversample=8, power_iterations=1, on_device=True)

        def by_gram():
            lam, Z = np.linalg.eigh(rec.data_gram())
            lam, Z = lam[::-1][:rank], Z[:, ::-1][:, :rank]
            s = np.sqrt(np.maximum(lam, 0.0))
            return Z, s, rec.jtvec_block([rec.unstack_data(Z[:, j] / s[j]) for j in range(rank)], on_device=True)
        per = {'sketch': [], 'gram': []}
        for r in range(repeat + 1):
            for key, f in (('sketch', by_sketch), ('gram', by_gram)):
                t, res = wall(f)
                if r:
                    per[key].append(t)
                if key == 'sketch':
                    s_sketch = res[1]
                else:
                    s_gram = res[1]
                del res
        k = min(len(s_sketch), len(s_gram))
        rel = np.abs(s_sketch[:k] - s_gram[:k]) / s_gram[0]
        say(f"  rank {rank:2d} (l = {min(rank + 8, M)}): sensitivity_svd {' '.join(f'{t:.2f}' for t in per['sketch'])} ms (mean "
            f"{np.mean(per['sketch']):.2f}); data_gram route {' '.join(f'{t:.2f}' for t in per['gram'])} ms (mean "
            f"{np.mean(per['gram']):.2f}); ratio of the means gram / sketch {np.mean(per['gram']) / np.mean(per['sketch']):.2f}; k = "
            f"{len(s_sketch)}, s_1 = {s_gram[0]:.3e}, s_k / s_1 = {s_gram[k - 1] / s_gram[0]:.2e}, max |s - s_gram| / s_1 = "
            f"{float(np.max(rel)):.2e} (largest at j = {int(np.argmax(rel)) + 1})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='marine128')
    ap.add_argument('--sources', type=int, default=4)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--launches', type=int, default=30, help="timed launches per kernel of the kernel block (>= 20)")
    ap.add_argument('--leg', choices=('all', 'products', 'hessian', 'gram', 'single', 'block', 'gnsolve', 'gndata', 'blocks',
                                     'svd'),
                    default='all',
                    help="products: the inner iteration four ways and its two reductions; hessian: hessian_diagonal against "
                         "the row-by-row route (needs only the set-up of ReciprocalSensitivity); gram: data_gram against the "
                         "route through jtvec, one frequency and two (the same set-up, once per survey); single: "
                         "field_dtype 'double' and 'single' side by side (not part of 'all'); block: K vectors per pass, the "
                         "block kernels and hessian_vec_block against K single calls (not part of 'all'); gnsolve: an "
                         "iteration of gauss_newton_solve, its kernels and the same iteration from torch operations (not "
                         "part of 'all'); gndata: the data-space preconditioner of gauss_newton_solve beside Jacobi (not part "
                         "of 'all'); blocks: the cell blocks of the Hessian beside its diagonal and block-Jacobi beside Jacobi "
                         "and the data-space preconditioner (not part of 'all'); svd: the kernels of the randomised SVD, the "
                         "orthonormalisation beside torch operations and sensitivity_svd beside the data_gram route (not part of "
                         "'all')")
    ap.add_argument('--field-dtype', choices=('double', 'single'), default='double',
                    help="how ReciprocalSensitivity keeps its fields in the reciprocal, hessian and gram legs")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sensitivity_times.txt'))
    ap.add_argument('--hessian-out', default=os.path.join(ROOT, 'profiles', 'hessian_diagonal_times.txt'))
    ap.add_argument('--gram-out', default=os.path.join(ROOT, 'profiles', 'data_gram_times.txt'))
    ap.add_argument('--single-out', default=os.path.join(ROOT, 'profiles', 'reciprocal_single_times.txt'))
    ap.add_argument('--block-out', default=os.path.join(ROOT, 'profiles', 'block_products_times.txt'))
    ap.add_argument('--gnsolve-out', default=os.path.join(ROOT, 'profiles', 'gauss_newton_solve_times.txt'))
    ap.add_argument('--weighted-out', default=os.path.join(ROOT, 'profiles', 'weighted_regulariser_times.txt'))
    ap.add_argument('--gndata-out', default=os.path.join(ROOT, 'profiles', 'data_preconditioner_times.txt'))
    ap.add_argument('--blocks-out', default=os.path.join(ROOT, 'profiles', 'hessian_blocks_times.txt'))
    ap.add_argument('--svd-out', default=os.path.join(ROOT, 'profiles', 'sensitivity_svd_times.txt'))
    args = ap.parse_args()
    K = args.sources
    wl = workload(args.workload)
    grid = emg3d.TensorMesh(wl['h'], wl['origin'])
    model = emg3d.Model(grid, **wl['res'])
    sources = {f'S{k}': workload(args.workload, source_index=k + 1, with_model=False)['source'] for k in range(K)}
    freqs = {'f': wl['frequency']}
    z = wl['source'][2]
    span = 0.25 * float(np.sum(wl['h'][0]))
    recs = np.array([[x, 0., z, 0., 0.] for x in np.linspace(-span, span, 8)])
    rng = np.random.default_rng(0)
    ncomp = {'isotropic': 1, 'VTI': 2, 'HTI': 2, 'triaxial': 3}[wl['case']]
    v = rng.standard_normal((ncomp,) + tuple(grid.shape_cells))
    y = {(s, 'f'): rng.standard_normal(len(recs)) + 1j * rng.standard_normal(len(recs)) for s in sources}
    lines = [f"# python tools/sensitivity_time.py --workload {args.workload} --sources {K} --repeat {args.repeat} --leg {args.leg}"
             f"{' --field-dtype single' if args.field_dtype == 'single' else ''}; box "
             f"{socket.gethostname()}, {torch.cuda.get_device_name(0)}; commit {commit()}, csrc_sha16 {csrc_sha16()}; "
             f"{time.strftime('%Y-%m-%d')}",
             f"# {wl['label']}; {K} sources x 1 frequency, {len(recs)} receivers; tol 1e-6, tol_gradient 1e-5, "
             "BiCGSTAB + multigrid; one inner iteration = jvec + jtvec; times in ms, synchronised"]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def hessian_leg(rec):
        head = [lines[0], f"# {wl['label']}; {K} sources x 1 frequency, {len(recs)} receivers; diag Re(J^H J) from the kept "
                          f"fields ({rec.kept_bytes:,} B), all weights one; times in ms, synchronised, results on the host"]
        first = len(lines)
        hessian_block(rec, say, args.repeat, args.launches)
        os.makedirs(os.path.dirname(os.path.abspath(args.hessian_out)), exist_ok=True)
        with open(args.hessian_out, 'w') as f:
            f.write('\n'.join(head + lines[first:]) + '\n')
        del lines[first:]

    def gram_leg(rec):
        """``rec``: the one-frequency object; the two-frequency one (the second at twice the frequency) is built here."""
        head = [lines[0], f"# {wl['label']}; {K} sources, {len(recs)} receivers; J^ J^T (all model weights one) from the kept "
                          "fields; route: 2 N jtvec calls + (Jhat * m) @ Jhat.T in NumPy; times in ms, synchronised, results "
                          "on the host"]
        first = len(lines)
        say(f"one frequency: M = {2 * len(rec.pairs) * len(recs)}, kept {rec.kept_bytes:,} B")
        gram_block(rec, say, args.repeat, args.launches, kernel=True)
        two = gradient.ReciprocalSensitivity(model, sources, {'f': wl['frequency'], 'g': 2 * wl['frequency']}, recs,
                                             solver_opts=dict(wl['opts'], tol=1e-6), keep='device', batch=K,
                                             field_dtype=args.field_dtype)
        two.forward()
        say(f"two frequencies ({wl['frequency']} and {2 * wl['frequency']} Hz): M = {2 * len(two.pairs) * len(recs)}, kept "
            f"{two.kept_bytes:,} B; three kernel calls (f-f, f-g, g-g)")
        gram_block(two, say, args.repeat, args.launches, kernel=False)
        two.release()
        os.makedirs(os.path.dirname(os.path.abspath(args.gram_out)), exist_ok=True)
        with open(args.gram_out, 'w') as f:
            f.write('\n'.join(head + lines[first:]) + '\n')
        del lines[first:]

    if args.leg == 'single':
        both = {}
        for name in ('double', 'single'):
            both[name] = gradient.ReciprocalSensitivity(model, sources, freqs, recs, solver_opts=dict(wl['opts'], tol=1e-6),
                                                        keep='device', batch=K, field_dtype=name)
            t0 = sync()
            both[name].forward()
            say(f"{name:7s} forward(): {1e3 * (sync() - t0):8.1f} ms; {both[name]!r}")
        single_block(both, say, args.repeat, args.launches, v, y)
        for rec in both.values():
            rec.release()
        os.makedirs(os.path.dirname(os.path.abspath(args.single_out)), exist_ok=True)
        with open(args.single_out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return
    if args.leg == 'block':
        for name in ('double', 'single'):
            kw = dict(solver_opts=dict(wl['opts'], tol=1e-6), batch=K, field_dtype=name)
            rec = gradient.ReciprocalSensitivity(model, sources, freqs, recs, keep='device', **kw)
            rec.forward()
            say(f"field_dtype='{name}': {rec!r}")
            block_kernels(rec, say, args.launches)
            say(f"methods, field_dtype='{name}' (wall time, synchronised, mean of {args.repeat} after a warm-up run, the two routes "
                "taking turns):")
            block_methods(rec, say, args.repeat, "keep='device'")
            rec.release()
            del rec
            host = gradient.ReciprocalSensitivity(model, sources, freqs, recs, keep='host', **kw)
            host.forward()
            block_methods(host, say, args.repeat, "keep='host'  ")
            host.release()
            del host
        os.makedirs(os.path.dirname(os.path.abspath(args.block_out)), exist_ok=True)
        with open(args.block_out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return
    if args.leg == 'gnsolve':
        lines[1] = (f"# {wl['label']}; {K} sources x 1 frequency, {len(recs)} receivers; (H + lambda_k R) x_k = b_k, K dampings over "
                    f"two decades, Jacobi, smallness {GN_REG[0]}, smoothness {GN_REG[1:]}, all weights one; times in ms")
        for name in ('double', 'single'):
            rec = gradient.ReciprocalSensitivity(model, sources, freqs, recs, solver_opts=dict(wl['opts'], tol=1e-6),
                                                 keep='device', batch=K, field_dtype=name)
            rec.forward()
            say(f"field_dtype='{name}': {rec!r}")
            gnsolve_block(rec, say, args.launches)
            if name == 'double':                                # the regulariser does not see the kept fields' type
                first = len(lines)
                say(f"weighted regulariser, weights uniform in [0.2, 5], u standard normal, eps {GN_EPS}; norms "
                    f"{', '.join(f'{a}: {b}' for a, b in GN_NORMS)}")
                weighted_block(rec, say, args.launches)
                weighted = lines[:2] + lines[first:]
                del lines[first:]
            rec.release()
            del rec
        os.makedirs(os.path.dirname(os.path.abspath(args.gnsolve_out)), exist_ok=True)
        with open(args.gnsolve_out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        with open(args.weighted_out, 'w') as f:
            f.write('\n'.join(weighted) + '\n')
        return
    if args.leg == 'gndata':
        lines[1] = (f"# {wl['label']}; {K} sources x 1 frequency, {len(recs)} receivers; (H + lambda_k R) x_k = b_k, the data-space "
                    f"(Woodbury) preconditioner beside Jacobi, smallness {GN_REG[0]}, smoothness {GN_REG[1:]}, all weights one, "
                    "field_dtype 'double'; times in ms")
        rec = gradient.ReciprocalSensitivity(model, sources, freqs, recs, solver_opts=dict(wl['opts'], tol=1e-6), keep='device',
                                             batch=K)
        rec.forward()
        say(f"{rec!r}")
        data_preconditioner_block(rec, say, args.launches)
        rec.release()
        os.makedirs(os.path.dirname(os.path.abspath(args.gndata_out)), exist_ok=True)
        with open(args.gndata_out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return
    if args.leg == 'blocks':
        lines[1] = (f"# {wl['label']}; {K} sources x 1 frequency, {len(recs)} receivers; the cell blocks of Re(J^H J) beside its "
                    f"diagonal, and (H + lambda_k R) x_k = b_k with block-Jacobi beside Jacobi and the data-space preconditioner, "
                    f"smallness {GN_REG[0]}, smoothness {GN_REG[1:]}, all weights one, field_dtype 'double'; times in ms")
        if ncomp < 2:
            raise SystemExit("--leg blocks needs a model with more than one property per cell (VTI, HTI, triaxial)")
        rec = gradient.ReciprocalSensitivity(model, sources, freqs, recs, solver_opts=dict(wl['opts'], tol=1e-6), keep='device',
                                             batch=K)
        rec.forward()
        say(f"{rec!r}")
        cell_blocks_block(rec, say, args.launches)
        rec.release()
        os.makedirs(os.path.dirname(os.path.abspath(args.blocks_out)), exist_ok=True)
        with open(args.blocks_out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return
    if args.leg == 'svd':
        lines[1] = (f"# {wl['label']}; {K} sources x 1 frequency, {len(recs)} receivers; the randomised truncated SVD of the "
                    "sensitivity, all weights one, field_dtype 'double'; times in ms")
        rec = gradient.ReciprocalSensitivity(model, sources, freqs, recs, solver_opts=dict(wl['opts'], tol=1e-6), keep='device',
                                             batch=K)
        rec.forward()
        say(f"{rec!r}")
        svd_block(rec, say, args.repeat, args.launches)
        rec.release()
        os.makedirs(os.path.dirname(os.path.abspath(args.svd_out)), exist_ok=True)
        with open(args.svd_out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return
    if args.leg in ('hessian', 'gram'):
        rec = gradient.ReciprocalSensitivity(model, sources, freqs, recs, solver_opts=dict(wl['opts'], tol=1e-6), keep='device',
                                             batch=K, field_dtype=args.field_dtype)
        rec.forward()
        (hessian_leg if args.leg == 'hessian' else gram_leg)(rec)
        rec.release()
        return
    variants = (("keep=False", dict(keep=False)), ("keep='device'", dict(keep='device')),
                (f"keep='device', batch={K}", dict(keep='device', batch=K)))
    lins, times = {}, {name: [] for name, _ in variants}
    for name, kw in variants:
        lin = lins[name] = gradient.Sensitivity(model, sources, freqs, recs, solver_opts=dict(wl['opts'], tol=1e-6), **kw)
        t0 = sync()
        lin.forward()
        t1 = sync()
        say(f"{name:28s} forward(): {1e3 * (t1 - t0):8.1f} ms (the first one builds the hierarchy); {lin!r}")
        setup = t1 - t0              # (of the last variant, keep='device', batch=K: what `reciprocal` is held against)
    rec = gradient.ReciprocalSensitivity(model, sources, freqs, recs, solver_opts=dict(wl['opts'], tol=1e-6), keep='device',
                                         batch=K, field_dtype=args.field_dtype)
    t0 = sync()
    rec.forward()
    t1 = sync()
    rname = 'reciprocal'
    say(f"{rname:28s} forward(): {1e3 * (t1 - t0):8.1f} ms = source solves {1e3 * rec.setup_seconds['forward']:8.1f} ms + "
        f"receiver solves {1e3 * rec.setup_seconds['receiver']:8.1f} ms (it_mg "
        f"{[rec.info[('receiver', r, 'f')]['it_mg'] for r in range(len(recs))]}); {rec!r}")
    rec_setup = t1 - t0
    times[rname] = []
    for r in range(args.repeat + 1):          # run 0: warm-up (coarse levels, line factors, graphs of the batch); the
        for name, _ in variants:              # variants take turns, so that a busy spell of the box hits all of them
            lin = lins[name]
            n0 = dict(lin.n_solves)
            t0 = sync()
            jv = lin.jvec(v)
            t1 = sync()
            jt = lin.jtvec(y)
            t2 = sync()
            solves = {k: lin.n_solves[k] - n0[k] for k in n0}
            its = [lin.info[p]['jvec']['it_mg'] for p in lin.pairs], [lin.info[p]['backward']['it_mg'] for p in lin.pairs]
            say(f"{name:28s} run {r}{' (warm-up)' if r == 0 else '':10s}: jvec {1e3 * (t1 - t0):8.1f}  jtvec "
                f"{1e3 * (t2 - t1):8.1f}  iteration {1e3 * (t2 - t0):8.1f} ms  solves {solves}  it_mg jvec {its[0]} jtvec {its[1]}"
                f"  |jvec| {np.linalg.norm(np.concatenate(list(jv.values()))):.6e} |jtvec| {np.linalg.norm(jt):.6e}")
            if r:
                times[name].append(t2 - t0)
        n0 = dict(rec.n_solves)
        t0 = sync()
        jv = rec.jvec(v)
        t1 = sync()
        jt = rec.jtvec(y)
        t2 = sync()
        say(f"{rname:28s} run {r}{' (warm-up)' if r == 0 else '':10s}: jvec {1e3 * (t1 - t0):8.3f}  jtvec "
            f"{1e3 * (t2 - t1):8.3f}  iteration {1e3 * (t2 - t0):8.3f} ms  solves { {k: rec.n_solves[k] - n0[k] for k in n0} }"
            f"  |jvec| {np.linalg.norm(np.concatenate(list(jv.values()))):.6e} |jtvec| {np.linalg.norm(jt):.6e}")
        if r:
            times[rname].append(t2 - t0)
    mean = {name: float(np.mean(t)) for name, t in times.items()}
    best = {name: float(np.min(t)) for name, t in times.items()}
    for lin in lins.values():
        lin.release()
    first, kept = "keep=False", "keep='device'"
    for name, t in mean.items():
        b = best[name]
        say(f"mean of {args.repeat}: {name:28s} {1e3 * t:8.2f} ms per inner iteration = {t / mean[first]:.4f} x keep=False, "
            f"{t / mean[kept]:.4f} x keep='device'  (fastest run {1e3 * b:8.2f} ms = {b / best[first]:.4f} x, "
            f"{b / best[kept]:.4f} x)")
    batched = f"keep='device', batch={K}"
    saving = mean[batched] - mean[rname]
    say(f"{rname}: set-up {1e3 * rec_setup:.1f} ms against {1e3 * setup:.1f} ms of {batched}: {1e3 * (rec_setup - setup):.1f} ms "
        f"more; inner iteration {1e3 * mean[rname]:.3f} ms against {1e3 * mean[batched]:.1f} ms: {1e3 * saving:.1f} ms less; "
        f"break-even after {(rec_setup - setup) / saving:.2f} inner iterations; kept {rec.kept_bytes:,} B")
    kernel_block(rec, say, args.launches)
    if args.leg == 'all':
        hessian_leg(rec)
        gram_leg(rec)
    rec.release()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
