"""Wall time of a Gauss-Newton inner iteration -- one ``jvec`` + one ``jtvec`` over K sources x 1 frequency of a bench
workload -- on one GPU, three ways: forward fields recomputed by every call (``keep=False``: the cost structure of
``misfit_and_gradient``), kept in HBM (``keep='device'``), and kept with the K right-hand sides solved together
(``keep='device', batch=K``). Writes profiles/sensitivity_times.txt.

    python tools/sensitivity_time.py [--workload marine128] [--sources 4] [--repeat 3] [--out profiles/sensitivity_times.txt]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='marine128')
    ap.add_argument('--sources', type=int, default=4)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sensitivity_times.txt'))
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
    lines = [f"# python tools/sensitivity_time.py --workload {args.workload} --sources {K} --repeat {args.repeat}; box "
             f"{socket.gethostname()}, {torch.cuda.get_device_name(0)}; commit {commit()}, csrc_sha16 {csrc_sha16()}; "
             f"{time.strftime('%Y-%m-%d')}",
             f"# {wl['label']}; {K} sources x 1 frequency, {len(recs)} receivers; tol 1e-6, tol_gradient 1e-5, "
             "BiCGSTAB + multigrid; one inner iteration = jvec + jtvec; times in ms, synchronised"]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    variants = (("keep=False", dict(keep=False)), ("keep='device'", dict(keep='device')),
                (f"keep='device', batch={K}", dict(keep='device', batch=K)))
    lins, times = {}, {name: [] for name, _ in variants}
    for name, kw in variants:
        lin = lins[name] = gradient.Sensitivity(model, sources, freqs, recs, solver_opts=dict(wl['opts'], tol=1e-6), **kw)
        t0 = sync()
        lin.forward()
        t1 = sync()
        say(f"{name:28s} forward(): {1e3 * (t1 - t0):8.1f} ms (the first one builds the hierarchy); {lin!r}")
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
    mean = {name: float(np.mean(t)) for name, t in times.items()}
    best = {name: float(np.min(t)) for name, t in times.items()}
    for lin in lins.values():
        lin.release()
    first, kept = "keep=False", "keep='device'"
    for name, t in mean.items():
        b = best[name]
        say(f"mean of {args.repeat}: {name:28s} {1e3 * t:8.1f} ms per inner iteration = {t / mean[first]:.3f} x keep=False, "
            f"{t / mean[kept]:.3f} x keep='device'  (fastest run {1e3 * b:8.1f} ms = {b / best[first]:.3f} x, "
            f"{b / best[kept]:.3f} x)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
