/*
 * emg3d_amd -- C ABI of the MI355X (gfx950) multigrid inner loop.
 *
 * Drop-in boundary for the hot path of emsig/emg3d: every entry point replaces one of the
 * numba kernels of the reference's emg3d/core.py (called from emg3d/solver.py at the
 * sites cited below) or one of the array-level pieces of emg3d/solver.py that have to live
 * on the device once the level hierarchy is device-resident.
 *
 * Two flavours:
 *   emg3d_core_*   HOST pointers, synchronous, exactly the arguments of the reference's
 *                  `core.<fn>` plus explicit sizes -- what a ctypes binding inside the
 *                  reference would call. Data is staged through HBM
 *                  per call; this flavour exists for parity tests and literal drop-in use.
 *   emg3d_dev_*    DEVICE pointers + hipStream_t, asynchronous; used by the device-resident
 *                  multigrid driver (emg3d_amd/solver.py).
 *
 * Conventions
 *   - All 3-D arrays are Fortran-ordered (x fastest), as in the reference
 *     (emg3d/fields.py:201-259): ex (nx,ny+1,nz+1), ey (nx+1,ny,nz+1), ez (nx+1,ny+1,nz),
 *     eta_x/eta_y/eta_z/zeta (nx,ny,nz). nx,ny,nz are CELL counts.
 *   - is_complex = 1: fields and eta are complex128 (interleaved re,im); 0: float64
 *     (Laplace domain, emg3d/fields.py:93-98). zeta and all widths/weights are float64.
 *   - eta_x, eta_y, eta_z may alias each other (isotropic / VTI / HTI models,
 *     emg3d/models.py:693-712); they are never written.
 *   - Return value: 0 on success, otherwise a HIP error code (hipError_t) or a negative
 *     emg3d_amd code; emg3d_last_error() gives the message. Numerical failure (zero
 *     pivot -> inf/nan) is NOT an error here, exactly as in the reference
 *     (emg3d/core.py:1560,1576); it surfaces through the residual norm.
 *   - Smoother ordering: four-colour ordering.
 *     point:  colour = ((ix+iz)&1) | (((iy+iz)&1)<<1);
 *     lines:  colour = (p&1) | ((q&1)<<1), (p,q) the transverse node indices in memory
 *             order: x-lines (iy,iz), y-lines (ix,iz), z-lines (ix,iy).
 *     Point smoother (option "point_order" = 1, the default since round 3): every sweep visits
 *     the node colours in the sequence 0,2,3,1 ("point_order" = 0: a backward sweep -- the
 *     first, third, ... sweep of a call, like the reference's backward-first alternation,
 *     emg3d/core.py:301,311 -- visits them in reverse: the rule of rounds 1-2, which needs up to
 *     a third more cycles). The sweep direction still reverses the TILE order of
 *     the tiled schedule below.
 *     Line smoothers (option "line_order" = 1, the default since round 3): the colour passes of
 *     a call cycle through the classes 1,2,3,0,1,2,3,0,...; sweep number it = 0,1,... of the call
 *     takes positions 3 it .. 3 it + 3 of that sequence (its first pass, for it > 0, repeats the
 *     class the previous sweep ended with: identical values, not launched). Measured on reduced
 *     copies of BASELINE.json's configurations this needs 12-18 % fewer cycles than mirrored
 *     sweeps at the same cost per cycle. "line_order" = 0: the mirrored sweeps
 *     0,2,3,1 / 1,3,2,0 (the lines' order in rounds 1-2). "line_order" = 2: the classes 1,2,3,0 in
 *     every sweep (4 nu launches per call instead of 3 nu + 1; one cycle in ten fewer at full size,
 *     a seventh more per smoothing call: equal in time).
 *     Point smoother on LARGE levels -- (nx-1)(ny-1)(nz-1) >= option "point_tile_min"
 *     (default 2^20) -- the interior nodes are cut into tiles of 32 x 4 x 6 nodes (tile t
 *     along an axis = nodes 1 + t*B .. (t+1)*B) which are coloured
 *     (tx&1)|((ty&1)<<1)|((tz&1)<<2); a forward sweep visits the tile colours in the order
 *     0,7,1,6,2,5,3,4 (backward: reversed; complementary colours are independent of each other
 *     and share a launch) and, inside every tile, the four node colours as above. This is the order in
 *     which one workgroup can keep a tile in LDS for all four node colours (one pass over
 *     the field per sweep instead of four); it is a Gauss-Seidel sweep like the others and
 *     converges alike. The oracle restates all of these orders.
 */
#ifndef EMG3D_AMD_H
#define EMG3D_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMG3D_AMD_VERSION 100 /* 0.1.0 */

#define EMG3D_ERR_BADARG (-1)
#define EMG3D_ERR_NODEVICE (-2)
#define EMG3D_ERR_SCRATCH (-3)
#define EMG3D_ERR_INTERNAL (-4) /* the library contradicted itself (a bug, not a caller's error) */

/* One grid level with device-resident arrays (emg3d_dev_* flavour). */
typedef struct emg3d_level {
    int32_t nx, ny, nz;        /* cells */
    int32_t is_complex;        /* 1 complex128, 0 float64 */
    void *ex, *ey, *ez;        /* electric field, updated in place by the smoothers */
    const void *sx, *sy, *sz;  /* source field */
    const void *eta_x, *eta_y, *eta_z;
    const double *zeta;
    const double *ihx, *ihy, *ihz; /* INVERSE cell widths 1/h (device) */
    /* Several right-hand sides that share the model (the sources of one frequency,
     * emg3d/simulations.py:1453-1464): batch > 1 of them are smoothed / reduced / transferred by
     * the same launches. Source b's buffers [ex|ey|ez] and [sx|sy|sz] start b * batch_stride
     * ELEMENTS behind source 0's (the pointers above). 0 or 1: a single source. */
    int32_t batch;
    int32_t flags;             /* EMG3D_LEVEL_* bits, 0 if unknown */
    int64_t batch_stride;
} emg3d_level;

/* emg3d_level::flags. ETA_IMAG: every eta value has a real part of exactly zero -- the
 * diffusive approximation at a real frequency, eta = -i omega mu0 sigma V (emg3d/models.py:
 * 677-678, epsilon_r is None). The tiled point smoother then keeps its eta edge sums as 8-byte
 * values (half the bytes, identical results). Never required; a caller that does not know
 * leaves it 0 or asks emg3d_dev_eta_is_imaginary. */
#define EMG3D_LEVEL_ETA_IMAG 1
/* LINE_COMPACT: the caller's promise that this level solves a CORRECTION equation -- its right-hand side is a
 * residual and its result is added to a field kept in full precision elsewhere (every coarse level of a cycle;
 * the finest level in residual form or as a Krylov preconditioner). The line passes that stream their records
 * through HBM (k_line_stream: lines of ~128 blocks and more) may then keep the inverse blocks T_k of the stored
 * factorisation and the forward pass's w records in SINGLE precision: values are rounded once when they are stored
 * and widened when they are loaded. The six right-hand-side entries r_Q of a line's middle block pass through the same
 * single-precision w scratch and are rounded once too (6e-8 relative, not multiplied by cond). Every operation, every
 * other right-hand side and the solution stay fp64. The fused kernel on shorter lines (k_line_colour) keeps the T_k in
 * single precision only: its w records and all of its right-hand sides, r_Q included, live in LDS as fp64. The line
 * solve becomes (A_line (1 + O(eps32 cond(S_k))))^-1 -- a perturbation of the smoother, not of the equation: the
 * iteration converges to the same field at the same rate as long as eps32 x cond of the 5 x 5 blocks (~ 1 / (omega mu
 * sigma h^2)) stays well below the smoothing factor, which is the caller's to check (emg3d_amd.solver: cond <= 3e4).
 * What it buys: 120 + 2 x 40 instead of 240 + 2 x 80 B per block and colour pass of the ~1 210 B such a pass moves,
 * and 184 instead of 304 B per cell and direction of factor memory. Set it BEFORE emg3d_dev_line_setup and keep it:
 * set-up, emg3d_line_fac_bytes_lv and the smoother read it from the level. Unset (0): everything fp64. */
#define EMG3D_LEVEL_LINE_COMPACT 2
/* POINT_COMPACT: the same promise (the level solves a correction equation) for the tiled point smoother: its eta edge
 * sums -- the imaginary (conduction) part of the diagonals of its 6 x 6 systems, emg3d/core.py:377-412, stored per
 * (tile, node colour, entry, thread) -- are kept in single precision: 24 instead of 48 B per node of the ~360 a sweep
 * moves (full values, with epsilon_r: 48 instead of 96). A relative perturbation of 6e-8 of those diagonal parts, i.e.
 * of the smoother, never of the residual the iteration is driven by. emg3d_point_compact_used says whether a level's
 * point smoother runs that way (flag set and the level large enough for the tiled schedule). */
#define EMG3D_LEVEL_POINT_COMPACT 4

int emg3d_version(void);
const char *emg3d_last_error(void);
/* number of visible HIP devices (0 without a GPU; never fails) */
int emg3d_device_count(void);
/* Run-time options. A name that is not in the list below is refused: emg3d_set_option returns EMG3D_ERR_BADARG,
 * emg3d_get_option returns -1. So is a value outside the stated set (the value then stays as it was), except where a
 * clamp is noted. Options marked (R) change results -- the order of the sweeps or a rounding; all others never do.
 *
 * Point smoother
 *   "point_tile_min" (R)  levels with at least this many interior nodes use the tiled schedule, which sweeps in
 *                         another order (see above). Default 1 << 20; <= 0 never, 1 always.
 *   "point_order" (R)     0 | 1: sequence of the node colours (see above).
 *   "point_compact" (R)   -1 | 0 | 1: single-precision eta sums of the tiled smoother: 0 (default) where the level asks
 *                         for them (EMG3D_LEVEL_POINT_COMPACT), 1 on every tiled level (tests, timing), -1 never.
 *   "point_slab"          plane-slab thickness of the plain launch schedule (0, default: one launch per colour over
 *                         all planes).
 *   "point_small"         levels with at most this many interior nodes (default 512; 0: off) run all passes of a call in
 *                         one single-workgroup launch.
 *   "tile_fuse"           1 (default): the tiles where two consecutive sweeps of a call meet run both sweeps on one LDS
 *                         copy (same operations, one load / store less); 0: every sweep on its own.
 *   "skip_repeat"         1 (default): the colour pass that repeats the last colour class of the previous sweep of the
 *                         same call is not launched (it reproduces the same values bit by bit); 0: every pass. Point
 *                         and line smoothers.
 * Line smoothers
 *   "line_order" (R)      0 | 1 | 2: sequence of the colour passes (see above).
 *   "line_wide" (R)       0 .. 64: lines of at most this many blocks (default 33; 0: never; only on levels small enough
 *                         to hold one more 16-entry record per block) are solved by k_line_wide: the same direct solve of
 *                         the line system (emg3d/core.py:1481-1616) with the same factors, the block recurrences
 *                         restated in four unknowns through N_k = (T_k C_k)[1..4, 1..4], one more rounding of T_k C_k --
 *                         fields agree with the other kernels' to rounding (~1e-13 per call), not bit for bit. A level
 *                         runs the same kernel for every right-hand side, so batched and separate solves stay bit-
 *                         identical under any value.
 *   "line_wide_bt"        0 | 192 | 256: block threads of a k_line_wide workgroup (0, default: whichever gives a
 *                         workgroup more lines).
 *   "line_compact" (R)    -1 | 0 | 1: single-precision line records: 0 (default) where the level asks for them
 *                         (EMG3D_LEVEL_LINE_COMPACT), 1 on every level whose kernels can read them (tests, timing),
 *                         -1 never.
 *   "line_fuse"           0: three launches per colour pass (right-hand sides, forward, backward); non-zero (default 2):
 *                         one fused launch -- the faster one at every size measured.
 *   "line_lds"            0 | 1: 1 (default) keeps the right-hand-side / solution records of a fused launch in LDS when
 *                         they fit, 0 always uses the global scratch.
 *   "line_lpw"            0 | 4 | 8 | 16 | 32: lines per workgroup of a fused launch (0, default: automatic; with 32 the
 *                         streamed kernel, whose two chain waves serve 16 lines, is not used).
 *   "line_stream"         2 (default): colour passes of lines whose records do not fit the LDS of a CU (~128 blocks and
 *                         more with 16 lines per workgroup) run k_line_stream -- right-hand sides, coupling entries and
 *                         w records staged through LDS rings by producer waves while the chain waves substitute
 *                         (bit-identical to the three-phase kernel); 1: only where not even slots 0..3 of the records
 *                         fit (~160 blocks and more); 0: the three-phase kernel everywhere.
 *   "line_stream_r"       rows per half of that ring: 0 (default: 16, and 8 for compact y / z lines) or a multiple of 4
 *                         in 4..32 (fewer where several right-hand sides share the LDS).
 *   "line_stream_bmin"    with several right-hand sides (emg3d_level::batch > 1) such passes on lines of at least this
 *                         many blocks (default 64; <= 0: never) serve GROUPS of up to four right-hand sides per
 *                         workgroup, every factor row fetched once per group (per source the same arithmetic: bit-
 *                         identical to separate solves) -- with the batch as a grid dimension every source's
 *                         workgroups fetch the factors again.
 * Residual
 *   "residual_zb"         planes a workgroup walks on large levels (default 8; values below 1 are clamped to 1).
 *   "residual_roll"       1 (default): operands a cell shares with the cell below it are carried in registers; 0: every
 *                         cell loads all of its own.
 * (Switches of earlier measurements that are gone: DESIGN.md, "Retired switches".) */
int emg3d_set_option(const char *name, int value);
int emg3d_get_option(const char *name);
/* enumeration of the options (for callers that key cached state -- captured graphs, option-
 * dependent buffers -- on the whole option set): names 0 .. emg3d_option_count()-1 */
int emg3d_option_count(void);
const char *emg3d_option_name(int i);
/* a counter that advances whenever emg3d_set_option changes a value: a cheap key for such caches */
int emg3d_options_generation(void);
/* The kernel that runs a colour pass of line direction lr (1/2/3) on a level of (nx,ny,nz) cells with
 * `batch` right-hand sides under the current options -- "k_line_stream" (records staged through an LDS
 * ring; with batch > 1: groups of right-hand sides per factor fetch), "k_line_colour" (three phases in one
 * launch) or the three separate kernels --, decided on the level's largest colour class by the very rule
 * the launcher uses. For profiles and benchmarks; "" on bad input. */
const char *emg3d_line_kernel_name(int lr, int nx, int ny, int nz, int is_complex, int batch);

/* ---------------------------------------------------------------- host flavour ---- */

/* core.amat_x (emg3d/core.py:57-206; called at emg3d/solver.py:695,1060):  r -= A e */
int emg3d_core_amat_x(void *rx, void *ry, void *rz, const void *ex, const void *ey, const void *ez,
                      const void *eta_x, const void *eta_y, const void *eta_z, const double *zeta,
                      const double *hx, const double *hy, const double *hz, int nx, int ny, int nz,
                      int is_complex);

/* core.gauss_seidel / _x / _y / _z (emg3d/core.py:210-1348; solver.py:837-846).
 * lr = 0 point, 1 x-line, 2 y-line, 3 z-line. */
int emg3d_core_gauss_seidel(int lr, void *ex, void *ey, void *ez, const void *sx, const void *sy,
                            const void *sz, const void *eta_x, const void *eta_y, const void *eta_z,
                            const double *zeta, const double *hx, const double *hy, const double *hz,
                            int nx, int ny, int nz, int nu, int is_complex);

/* core.restrict (emg3d/core.py:1620-2001; solver.py:937). Coarse/fine NODE counts are
 * implied: fine cells (nx,ny,nz), coarse cells = fine/2 in every coarsened direction.
 * w?l/w?0/w?r: weights of emg3d/core.py:2004-2076 (length = coarse nodes; ignored for a
 * direction that sc_dir does not coarsen). */
int emg3d_core_restrict(void *crx, void *cry, void *crz, const void *rx, const void *ry,
                        const void *rz, const double *wxl, const double *wx0, const double *wxr,
                        const double *wyl, const double *wy0, const double *wyr, const double *wzl,
                        const double *wz0, const double *wzr, int nx, int ny, int nz, int sc_dir,
                        int is_complex);

/* core.blocks_to_amat (emg3d/core.py:1351-1477) and core.solve (emg3d/core.py:1481-1616)
 * on the reference's banded storage A(i,j) -> amat[i+5j]. Inside the line smoothers these
 * never exist (the factorisation is streamed); the entry points are kept for the
 * reference's known-answer tests and run as single-thread device kernels. */
int emg3d_core_blocks_to_amat(void *amat, void *bvec, const void *middle, const double *left,
                              const void *rhs, int im, int nc, int n, int is_complex);
int emg3d_core_solve(void *amat, void *bvec, int n, int is_complex);

/* -------------------------------------------------------------- device flavour ---- */

/* Line relaxation keeps the block factorisation of every line matrix in HBM: it depends
 * on eta, zeta and h only, so it is computed once per level and direction
 * (emg3d_dev_line_setup) and reused by every sweep -- the work core.solve
 * (emg3d/core.py:1481-1616) repeats on every call of the reference's line smoothers.
 * Accuracy: the local systems are as ill-conditioned as 1 / (omega mu sigma h^2) (1e5 in sediments
 * at 1 Hz, 5e9 in air of 1e8 Ohm m), so any two fp64 evaluations of a sweep differ by eps x cond:
 * 1e-14 (marine model) ... 3e-6 (the same model under an air layer, random fields) between these
 * kernels -- point and line smoothers alike -- and the reference's arithmetic. What sets the line
 * smoothers apart is the RESIDUAL a solve leaves: multiplying by the stored inverses of the 5 x 5
 * Schur complements it is eps x cond x |right-hand side|, where a substitution (the point
 * smoother's, the reference's) leaves eps x |right-hand side|. An iteration whose tolerance is below
 * that runs the smoother on the residual equation (emg3d_amd.solve(residual_form=...) on the finest
 * level; coarse levels and preconditioner calls are in that form anyway): the errors then scale
 * with the residual and the iteration converges to round-off.
 * Sizes of the two factor buffers (complex/real part `fac`, real coupling part `lfac`)
 * and of the per-call scratch (right-hand sides / solutions of one colour class): */
size_t emg3d_line_fac_bytes(int lr, int nx, int ny, int nz, int is_complex);
/* ... of `fac` for THIS level: smaller where its direction lr keeps compact records (EMG3D_LEVEL_LINE_COMPACT and the
 * direction streams; emg3d_line_compact_used says whether), else emg3d_line_fac_bytes -- which is always enough */
size_t emg3d_line_fac_bytes_lv(const emg3d_level *lv, int lr);
int emg3d_line_compact_used(const emg3d_level *lv, int lr);
int emg3d_point_compact_used(const emg3d_level *lv);
size_t emg3d_line_lfac_bytes(int lr, int nx, int ny, int nz);
size_t emg3d_gs_scratch_bytes(int lr, int nx, int ny, int nz, int is_complex); /* 0 for lr = 0 */

/* Factorise all lines of direction lr (1/2/3 = x/y/z) of level lv into fac / lfac. */
int emg3d_dev_line_setup(const emg3d_level *lv, int lr, void *fac, double *lfac, void *stream);

/* Point smoother: the eta edge sums of emg3d/core.py:377-390 (one value per edge, arrays
 * shaped like ex|ey|ez) depend on the model only; computed once per level they replace 24
 * scattered eta loads per node by 6. Optional: emg3d_dev_gauss_seidel(lr = 0) forms the sums
 * on the fly when fac == NULL; both give identical bits. */
size_t emg3d_point_fac_bytes(int nx, int ny, int nz, int is_complex);   /* upper bound (flags = 0) */
size_t emg3d_point_fac_bytes_lv(const emg3d_level *lv);                  /* exact, honours lv->flags */
int emg3d_dev_point_setup(const emg3d_level *lv, void *fac, void *stream);
/* On levels that use the tiled schedule (option "point_tile_min", which must not change between
 * setup and use) the sums are laid out tile by tile, node colour by node colour, so that every
 * colour step of a workgroup reads them as one dense stream and every byte once per sweep; each
 * edge sum then exists twice (once per end node): 96 B per node, or 48 B with
 * EMG3D_LEVEL_ETA_IMAG / real fields. Elsewhere: arrays shaped like ex|ey|ez.
 *
 * *result = 1 if all real parts of lv's eta arrays are exactly zero (synchronises `stream`). */
int emg3d_dev_eta_is_imaginary(const emg3d_level *lv, int *result, void *stream);

/* nu sweeps of the smoother lr (0 point, 1/2/3 line along x/y/z) on level lv.
 * fac/lfac: from emg3d_dev_line_setup for the same level and lr; for lr = 0 fac is the
 * buffer of emg3d_dev_point_setup or NULL, lfac is ignored. With lv->batch > 1 all right-hand
 * sides are swept by the same launches (the factors are shared); scratch must then hold
 * batch x emg3d_gs_scratch_bytes. */
int emg3d_dev_gauss_seidel(const emg3d_level *lv, int lr, int nu, const void *fac, const double *lfac,
                           void *scratch, size_t scratch_bytes, void *stream);

/* Number of doubles of workspace emg3d_dev_residual needs for its block partial sums. */
size_t emg3d_residual_ws_len(int nx, int ny, int nz);

/* solver.residual (emg3d/solver.py:1022-1070): r = s - A e for the whole buffer
 * (rx/ry/rz may be NULL: norm only; they may alias lv->s*: in-place core.amat_x form).
 * If sumsq != NULL, *sumsq (device double) receives sum |r|^2 over all entries
 * (deterministic two-stage reduction through ws). With lv->batch > 1: r buffers stacked like
 * the fields (batch_stride), ws of batch x emg3d_residual_ws_len doubles, sumsq[batch]. */
int emg3d_dev_residual(const emg3d_level *lv, void *rx, void *ry, void *rz, double *ws,
                       size_t ws_len, double *sumsq, void *stream);

/* core.restrict on device pointers; fine cells (nx,ny,nz). w arrays are device pointers. */
int emg3d_dev_restrict(void *crx, void *cry, void *crz, const void *rx, const void *ry,
                       const void *rz, const double *wxl, const double *wx0, const double *wxr,
                       const double *wyl, const double *wy0, const double *wyr, const double *wzl,
                       const double *wz0, const double *wzr, int nx, int ny, int nz, int sc_dir,
                       int is_complex, void *stream);

/* solver.prolongation (emg3d/solver.py:947-1019): fine e += P coarse e, interior only.
 * il?/w? (device, length fine nodes): lower coarse node and weight of the upper coarse
 * node per fine node (emg3d/solver.py:1457-1462). */
int emg3d_dev_prolong(void *ex, void *ey, void *ez, const void *cex, const void *cey, const void *cez,
                      const int32_t *ilx, const int32_t *ily, const int32_t *ilz, const double *wx,
                      const double *wy, const double *wz, int nx, int ny, int nz, int sc_dir,
                      int is_complex, void *stream);

/* The two transfers for `batch` right-hand sides stacked like emg3d_level::batch describes:
 * source b's fine buffers start b * fine_stride elements behind source 0's, its coarse buffers
 * b * coarse_stride; one launch serves all of them. */
int emg3d_dev_restrict_batch(void *crx, void *cry, void *crz, const void *rx, const void *ry,
                             const void *rz, const double *wxl, const double *wx0, const double *wxr,
                             const double *wyl, const double *wy0, const double *wyr, const double *wzl,
                             const double *wz0, const double *wzr, int nx, int ny, int nz, int sc_dir,
                             int is_complex, int batch, size_t fine_stride, size_t coarse_stride,
                             void *stream);
/* the same restriction that also sets the coarse FIELD ce* to zero -- the start value of the coarse
 * solve (emg3d/solver.py:941) -- in the same pass over the coarse edges (no separate fill launch) */
int emg3d_dev_restrict_clear_batch(void *crx, void *cry, void *crz, void *cex, void *cey, void *cez,
                                   const void *rx, const void *ry, const void *rz, const double *wxl,
                                   const double *wx0, const double *wxr, const double *wyl,
                                   const double *wy0, const double *wyr, const double *wzl,
                                   const double *wz0, const double *wzr, int nx, int ny, int nz,
                                   int sc_dir, int is_complex, int batch, size_t fine_stride,
                                   size_t coarse_stride, void *stream);
int emg3d_dev_prolong_batch(void *ex, void *ey, void *ez, const void *cex, const void *cey,
                            const void *cez, const int32_t *ilx, const int32_t *ily, const int32_t *ilz,
                            const double *wx, const double *wy, const double *wz, int nx, int ny, int nz,
                            int sc_dir, int is_complex, int batch, size_t fine_stride,
                            size_t coarse_stride, void *stream);

/* solver._restrict_model_parameters (emg3d/solver.py:1667-1718): coarse = sum of the
 * 2/4/8 fine cells; is_complex refers to the parameter dtype (eta: field dtype, zeta: 0). */
int emg3d_dev_restrict_param(void *out, const void *in, int nx, int ny, int nz, int sc_dir,
                             int is_complex, void *stream);

/* Zero the tangential field on the six PEC faces (emg3d/solver.py:349-355). */
int emg3d_dev_pec_zero(void *ex, void *ey, void *ez, int nx, int ny, int nz, int is_complex,
                       void *stream);

/* ---- around the multigrid cycle: Krylov vector work -------------------
 * solver.krylov (emg3d/solver.py:652-784) wraps scipy.sparse.linalg.{bicgstab, cgs} around the
 * multigrid preconditioner; their vector updates and inner products run on the device as
 * instances of one fused step,
 *     y = sum_{i < nterms} c_i xs[i]         c_i = table[slots[i]] * scales[i], or scales[i] alone
 *                                            if slots[i] < 0;  y may be one of the xs; nterms <= 4
 *     table[dslots[k]] = conj(das[k]) . dbs[k]   for k < ndots <= 3, evaluated with the new y
 * followed by up to 8 scalar instructions prog[4 i .. 4 i + 3] = (op, dst, a, b) on the table:
 * op 0 dst = a / b, 1 dst = a * b, 2 dst = -a, 3 dst = a. `table` holds complex scalars as
 * (re, im) pairs of doubles in device memory (real fields use the real parts), so the scalars
 * of the recurrences stay on the GPU; the host reads the table when it has to decide
 * (convergence, breakdown). ws: emg3d_krylov_ws_len() doubles. Vectors have n entries of the
 * field dtype; the arrays of pointers / integers / scales are HOST arrays. */
size_t emg3d_krylov_ws_len(void);
int emg3d_dev_krylov_step(size_t n, int is_complex, void *y, int nterms, const void *const *xs, const int *slots,
                          const double *scales, int ndots, const void *const *das, const void *const *dbs,
                          const int *dslots, int nprog, const int *prog, double *table, double *ws, size_t ws_len,
                          void *stream);
/* The Krylov operator (emg3d/solver.py:686-702): out = A x with x = lv->ex|ey|ez (lv->s* unused);
 * entries core.amat_x never touches (upper boundary) are set to zero. */
int emg3d_dev_apply_operator(const emg3d_level *lv, void *ox, void *oy, void *oz, void *stream);
/* zero fill (a kernel of the library: as a hipMemsetAsync node of a captured graph it was seen to
 * race with the neighbouring kernels) / device-to-device hipMemcpyAsync, on the stream */
int emg3d_dev_zero(void *p, size_t bytes, void *stream);
int emg3d_dev_copy(void *dst, const void *src, size_t bytes, void *stream);

/* ---- after a solve: magnetic field and receiver responses ------------
 * fields.get_magnetic_field / _edge_curl_factor (emg3d/fields.py:617-659, 941-1009):
 * m = curl(e) * (zeta / (s mu0)) averaged over the two cells of a face, on the faces
 * mx (nx+1,ny,nz), my (nx,ny+1,nz), mz (nx,ny,nz+1); boundary faces stay 0. zeta = V / mu_r
 * (nx,ny,nz) doubles, hx/hy/hz cell widths -- all device pointers; s mu0 = smu0_re + i smu0_im
 * (real fields: smu0_im ignored). */
int emg3d_dev_magnetic_field(int nx, int ny, int nz, int is_complex, const void *ex, const void *ey,
                             const void *ez, const double *zeta, const double *hx, const double *hy,
                             const double *hz, double smu0_re, double smu0_im, void *mx, void *my,
                             void *mz, void *stream);

/* fields.get_receiver -> maps.interpolate (emg3d/fields.py:522-614, emg3d/maps.py:232-368).
 * method 'cubic' = maps.interp_spline_3d (maps.py:500-552) = scipy.ndimage.map_coordinates(
 * order=3, mode='constant', cval=nan): emg3d_dev_spline_filter turns the n0 x n1 x n2 array
 * (x fastest) IN PLACE into cubic B-spline coefficients (scipy.ndimage.spline_filter, mirror);
 * emg3d_dev_spline_eval evaluates them at npts index-space coordinates coords[0..npts) = x,
 * [npts..2npts) = y, [2npts..3npts) = z (the host maps metres to index space with the same 1-D
 * cubic interpolant as the reference); points outside [0, n-1] give NaN. */
int emg3d_dev_spline_filter(void *data, int n0, int n1, int n2, int is_complex, void *stream);
int emg3d_dev_spline_eval(const void *coef, int n0, int n1, int n2, int is_complex,
                          const double *coords, int npts, void *out, void *stream);
/* method 'linear' = scipy RegularGridInterpolator(fill_value=nan): idx (3 x npts, int32) is the
 * lower corner of the cell holding each point (any entry < 0: outside, NaN), w (3 x npts) the
 * weights of the upper corner. */
int emg3d_dev_linear_eval(const void *values, int n0, int n1, int n2, int is_complex,
                          const int32_t *idx, const double *w, int npts, void *out, void *stream);

/* ---- adjoint-state gradient ---------------------------------------------
 * Simulation.gradient (emg3d/simulations.py:1041-1063) per source-frequency pair:
 * gfield = real(bfield * s mu0 * efield) on the edges, maps.interp_edges_to_vol_averages
 * (emg3d/maps.py:667-719) to the cells, added to the gradient -- one kernel over the cells with
 * the forward field e* and the back-propagated field b* in HBM. volumes (nx,ny,nz), g* (nx,ny,nz)
 * doubles, accumulated (+=): the three components of the reference's (3, nx, ny, nz) array. */
int emg3d_dev_gradient_accumulate(int nx, int ny, int nz, int is_complex, const void *ex, const void *ey,
                                  const void *ez, const void *bx, const void *by, const void *bz,
                                  double smu0_re, double smu0_im, const double *volumes, double *gx,
                                  double *gy, double *gz, void *stream);

/* ---- sensitivity products: the source of Simulation.jvec (emg3d/simulations.py:1352-1362) -----
 * The transpose of emg3d_dev_gradient_accumulate: a model perturbation v* (cells, doubles, one array
 * per component; vy / vz may alias vx) becomes a source field on the edges,
 *     g = -s mu0 * e * 1/4 * sum over the (up to four) cells that share the edge of volumes * v
 * (the reference takes the operator from discretize's get_edge_inner_product_deriv). g* is WRITTEN
 * (every edge, not accumulated) and may be any device buffer laid out like a field -- in practice a
 * level's source vector, or slice b of it for a batch. Fixed summation order (cells z outer, y, x
 * inner), no atomics. For any fields e, b and real v:
 *     sum_cells v_k * gradient_accumulate(e, b)_k == -Re sum_edges b * sensitivity_source(e, v). */
int emg3d_dev_sensitivity_source(int nx, int ny, int nz, int is_complex, const void *ex, const void *ey,
                                 const void *ez, double smu0_re, double smu0_im, const double *volumes,
                                 const double *vx, const double *vy, const double *vz, void *gx, void *gy,
                                 void *gz, void *stream);

/* ---- solve-free sensitivity products from kept source AND receiver fields --------
 * The system matrix is complex symmetric and the receiver operator does not depend on the source, so
 * with one kept field per source, e_s, and one per receiver, x_r = A^-1 (the residual source of a unit
 * datum at receiver r alone), both products of gradient.ReciprocalSensitivity are reductions over the
 * kept fields:
 *     jvec(v)_{s,r} = c sum_k w_k e_s[k] x_r[k]          w = emg3d_dev_edge_weights(v), c = conj(-s mu0)
 *     jtvec(y)      = edges_to_cells(t),                  t[k] = sum_s e_s[k] sum_r conj(y_{s,r}) x_r[k]
 * Fields of one kind are STACKED like emg3d_level::batch: field i starts i * stride elements behind
 * field 0, stride >= n (what lies between n and stride is never read); elements are complex128
 * (is_complex) or float64. Plain fp64, no atomics, every sum in a fixed order that depends on the sizes
 * alone: the same call gives the same bits.
 *
 * emg3d_dev_edge_weights: emg3d_dev_sensitivity_source without the field,
 *     w = 1/4 * sum over the (up to four) cells that share the edge of volumes * v,
 * WRITTEN to w* (laid out like a real field); cells in the same order, vy / vz may alias vx. */
int emg3d_dev_edge_weights(int nx, int ny, int nz, const double *volumes, const double *vx,
                           const double *vy, const double *vz, double *wx, double *wy, double *wz,
                           void *stream);
/* out[s * nr + r] = scale * sum_k w[k] e_s[k] x_r[k] (out: device, ns * nr elements, written). A
 * tall-skinny GEMM with K = n, bound by HBM: workgroups stream 8192 consecutive k for a 4 x 4 tile of
 * (s, r) with the accumulators in registers, reduce in the wave, through LDS, and across workgroups
 * through ws (doubles, at least emg3d_sensitivity_dots_ws_len(ns, nr, n) of them) in a second launch.
 * Fields read: e ceil(nr / 4) times, x ceil(ns / 4) times. ns, nr >= 1, otherwise unbounded. */
size_t emg3d_sensitivity_dots_ws_len(int ns, int nr, size_t n);
int emg3d_dev_sensitivity_dots(size_t n, int is_complex, const void *e, size_t e_stride, int ns,
                               const void *x, size_t x_stride, int nr, const double *w, double scale_re,
                               double scale_im, void *out, double *ws, size_t ws_len, void *stream);
/* t[k] = sum_s e_s[k] * (sum_r coef[s * nr + r] * x_r[k]), r first, then s, both ascending; t (n
 * elements) is WRITTEN. coef: device, ns * nr elements of the fields' type. One pass: every e_s once,
 * every x_r once (beyond 8 receivers the further ones once per source). */
int emg3d_dev_sensitivity_combine(size_t n, int is_complex, const void *e, size_t e_stride, int ns,
                                  const void *x, size_t x_stride, int nr, const void *coef, void *t,
                                  void *stream);
/* emg3d_dev_gradient_accumulate with the edge product t = b * e already formed:
 * g += volume / 4 * sum real(s mu0 * t) over a cell's four x-, y- and z-edges, in the same order. */
int emg3d_dev_edges_to_cells(int nx, int ny, int nz, int is_complex, const void *tx, const void *ty,
                             const void *tz, double smu0_re, double smu0_im, const double *volumes,
                             double *gx, double *gy, double *gz, void *stream);
/* Diagonal of the Gauss-Newton Hessian, diag Re(J^H W J), from the same kept stacks:
 * the Jacobian row of datum (s, r) w.r.t. the conductivity component d of cell c is
 * s mu0 V_c / 4 Z_{s,r,d}(c), Z = sum of e_s[k] x_r[k] over the four d-edges of c (those of
 * emg3d_dev_edges_to_cells, in its order), so
 *     h[p * h_stride + c] += scale (V_c / 4)^2 sum_{s,r} weights[s * nr + r]
 *                                               | sum_{d: row_d = p} Z_{s,r,d}(c) |^2 ,
 * components with the same row added BEFORE the modulus (isotropic (0,0,0), HTI (0,1,0), VTI (0,0,1),
 * tri-axial (0,1,2)); scale = |s mu0|^2. e, x: stacks as above, every field [x-edges | y-edges |
 * z-edges], strides >= n_edges; weights: device, ns * nr doubles >= 0; h: rows 0..max(row) of n_cells
 * doubles (x fastest), h_stride >= n_cells apart, ACCUMULATED into -- rows that no direction maps to
 * are not touched. One pass: a workgroup stages the edges of a patch of cells for a tile of sources
 * and receivers in LDS and keeps the tile's pair sums and the three row sums of its cells in registers
 * (csrc/hessian.h). Plain fp64, no atomics, sums in an order fixed by the sizes. */
int emg3d_dev_hessian_diagonal(int nx, int ny, int nz, int is_complex, const void *e, size_t e_stride,
                               int ns, const void *x, size_t x_stride, int nr, const double *weights,
                               int row_x, int row_y, int row_z, double scale, const double *volumes,
                               double *h, size_t h_stride, void *stream);
/* The n x n blocks of the Gauss-Newton Hessian that couple the components of ONE cell,
 * n = max(row) + 1: with Z_p = sum_{d: row_d = p} Z_{s,r,d}(c) of emg3d_dev_hessian_diagonal,
 *     h[m * h_stride + c] += scale (V_c / 4)^2 sum_{s,r} weights[s * nr + r] Re( conj(Z_p) Z_q )
 * (real fields: Z_p Z_q) for the n (n + 1) / 2 packed rows m = (p, q), p <= q: the diagonal (0,0) ..
 * (n-1,n-1) first -- what emg3d_dev_hessian_diagonal adds --, then (0,1) and, for n = 3, (0,2), (1,2).
 * Arguments and checks as there; in addition every row below n must have a direction: a row map such
 * as (0, 2, 2) is EMG3D_ERR_BADARG. n = 1: one row, the diagonal. One pass over the stacks, the same
 * bytes as the diagonal: every direction is staged once per tile of sources and receivers and the pair
 * sums of all rows stay in registers (csrc/hessian_blocks.h; n = 3 works on tiles of 4 x 2). Plain
 * fp64, no atomics, sums in an order fixed by the sizes. */
int emg3d_dev_hessian_cell_blocks(int nx, int ny, int nz, int is_complex, const void *e, size_t e_stride,
                                  int ns, const void *x, size_t x_stride, int nr, const double *weights,
                                  int row_x, int row_y, int row_z, double scale, const double *volumes,
                                  double *h, size_t h_stride, void *stream);
/* One block of the data-space Gauss-Newton matrix G^ = J^ diag(m) J^T between the data
 * of a side A and a side B -- two frequencies, or one and the same --, from the kept stacks of either
 * side (conventions as above). J^ has the rows Re J_i, i = s * nr + r, and, for complex fields (c = 2;
 * real fields: c = 1), behind them the rows Im J_i. out[i * ld + j], i < c ns_a nr_a, j < c ns_b nr_b,
 * is WRITTEN (entries between a row's end and ld are not touched):
 *     out[i, j] = sum_{p, cell} mw[p * mw_stride + cell] (V_cell / 4)^2 a^_{i,p}(cell) b^_{j,p}(cell),
 * a^ = real part (first half of the rows, s-major) or imaginary part (second half) of
 * scale_a * sum_{d: row_d = p} Z^A_{s,r,d}(cell), b^ the same of side B; Z: the pair sum of
 * emg3d_dev_hessian_diagonal (same four edges per direction, same order); scale: the frequency's
 * s mu0 (real fields: scale_re); model_weights: device, rows 0..max(row) of n_cells doubles >= 0,
 * mw_stride >= n_cells apart, already model weights * chain^2. ws: device,
 * >= emg3d_data_gram_ws_len(nx, ny, nz, is_complex, ns_a * nr_a, ns_b * nr_b) doubles (0: bad sizes).
 * Two launches (csrc/gram.h): workgroups that own a pair of 32-datum tiles generate the rows of J^ for
 * a patch of cells in LDS and consume them in a rank update held in registers; their partial tiles go
 * to ws and are added in ascending order. Plain fp64, no atomics, every sum in an order fixed by the
 * sizes alone. With the same stacks, strides, counts and scales on both sides the block is bitwise
 * symmetric: one triangle of tile pairs is computed and mirrored. */
size_t emg3d_data_gram_ws_len(int nx, int ny, int nz, int is_complex, int n_a, int n_b);
int emg3d_dev_data_gram(int nx, int ny, int nz, int is_complex, const void *e_a, size_t e_a_stride,
                        int ns_a, const void *x_a, size_t x_a_stride, int nr_a, double scale_a_re,
                        double scale_a_im, const void *e_b, size_t e_b_stride, int ns_b, const void *x_b,
                        size_t x_b_stride, int nr_b, double scale_b_re, double scale_b_im, int row_x,
                        int row_y, int row_z, const double *model_weights, size_t mw_stride,
                        const double *volumes, double *out, size_t ld, double *ws, size_t ws_len,
                        void *stream);

/* ---- kept fields stored in single precision ---------------------------------------
 * The four products above for stacks that are STORED narrow: elements are complex64 (is_complex: two
 * floats, re then im) or float32. Each entry takes the argument list of its sibling and returns its
 * errors with its texts; strides count elements of the narrow type. Only the stacks are narrow. Every
 * value is widened when it is loaded and every operation, partial sum and result is fp64 as in the
 * sibling; emg3d_sensitivity_dots_ws_len and emg3d_data_gram_ws_len serve both variants. No atomics,
 * sums in a fixed order: the same call gives the same bits.
 *
 * emg3d_dev_sensitivity_dots_sp: NARROW e, x. fp64: w, scale, out (ns * nr complex128 / float64), ws.
 * Where e, x and w and both strides are multiples of 16 bytes a lane takes 16 bytes (two complex64 or
 * four float32, consecutive k) per field and load, otherwise one element; the order of the sum is a
 * function of the sizes and of that one bit. What lies between n and a stride is never read. */
int emg3d_dev_sensitivity_dots_sp(size_t n, int is_complex, const void *e, size_t e_stride, int ns,
                                  const void *x, size_t x_stride, int nr, const double *w,
                                  double scale_re, double scale_im, void *out, double *ws, size_t ws_len,
                                  void *stream);
/* emg3d_dev_sensitivity_combine_sp: NARROW e, x. fp64: coef (ns * nr complex128 / float64) and t (n
 * complex128 / float64, WRITTEN). 16-byte loads under the rule above (t in the place of w); t does not
 * depend on which loads are used. */
int emg3d_dev_sensitivity_combine_sp(size_t n, int is_complex, const void *e, size_t e_stride, int ns,
                                     const void *x, size_t x_stride, int nr, const void *coef, void *t,
                                     void *stream);
/* emg3d_dev_hessian_diagonal_sp: NARROW e, x. fp64: weights, scale, volumes, h. The edges of a patch
 * are staged in LDS as stored (half the LDS of the sibling) and widened when they are used. */
int emg3d_dev_hessian_diagonal_sp(int nx, int ny, int nz, int is_complex, const void *e, size_t e_stride,
                                  int ns, const void *x, size_t x_stride, int nr, const double *weights,
                                  int row_x, int row_y, int row_z, double scale, const double *volumes,
                                  double *h, size_t h_stride, void *stream);
/* emg3d_dev_hessian_cell_blocks_sp: NARROW e, x; everything else as for emg3d_dev_hessian_diagonal_sp. */
int emg3d_dev_hessian_cell_blocks_sp(int nx, int ny, int nz, int is_complex, const void *e, size_t e_stride,
                                     int ns, const void *x, size_t x_stride, int nr, const double *weights,
                                     int row_x, int row_y, int row_z, double scale, const double *volumes,
                                     double *h, size_t h_stride, void *stream);
/* emg3d_dev_data_gram_sp: NARROW e_a, x_a, e_b, x_b (both sides). fp64: the scales, model_weights,
 * volumes, out, ws. Staging as in emg3d_dev_hessian_diagonal_sp; the panels are fp64. */
int emg3d_dev_data_gram_sp(int nx, int ny, int nz, int is_complex, const void *e_a, size_t e_a_stride,
                           int ns_a, const void *x_a, size_t x_a_stride, int nr_a, double scale_a_re,
                           double scale_a_im, const void *e_b, size_t e_b_stride, int ns_b,
                           const void *x_b, size_t x_b_stride, int nr_b, double scale_b_re,
                           double scale_b_im, int row_x, int row_y, int row_z,
                           const double *model_weights, size_t mw_stride, const double *volumes,
                           double *out, size_t ld, double *ws, size_t ws_len, void *stream);

/* ---- block sensitivity products: nv vectors per pass over the kept stacks ----------
 * emg3d_dev_sensitivity_dots and emg3d_dev_sensitivity_combine for nv >= 1 vectors at once; stacks,
 * strides and types as there. A field value is loaded once for all the vectors of a tile (csrc/block.h).
 * Plain fp64, no atomics, every sum in an order fixed by the sizes alone: the same call gives the same
 * bits. Sizes beyond one launch are refused with EMG3D_ERR_BADARG.
 *
 * out[(v * ns + s) * nr + r] = scale * sum_k w_v[k] e_s[k] x_r[k] (out: device, nv * ns * nr elements of
 * the fields' type, written). w: nv rows of n doubles, row v starts v * w_stride doubles behind row 0,
 * w_stride >= n (what lies between n and w_stride is never read). A wave streams 4096 consecutive k for
 * a tile of 2 x 4 (s, r) and 4 vectors: the products e_s[k] x_r[k] are formed once per k and added into
 * the accumulators of the 4 vectors, in registers; the up to 8 waves of a workgroup take different tiles
 * of the same k, so that a field value comes from HBM once. Reduced in the wave and across workgroups
 * through ws (doubles, at least emg3d_sensitivity_dots_block_ws_len(ns, nr, nv, n) of them; 0: bad
 * sizes) in a second launch. Equal to emg3d_dev_sensitivity_dots per vector up to the order of the sums
 * (nv = 1 runs that kernel). */
size_t emg3d_sensitivity_dots_block_ws_len(int ns, int nr, int nv, size_t n);
int emg3d_dev_sensitivity_dots_block(size_t n, int is_complex, const void *e, size_t e_stride, int ns,
                                     const void *x, size_t x_stride, int nr, const double *w,
                                     size_t w_stride, int nv, double scale_re, double scale_im, void *out,
                                     double *ws, size_t ws_len, void *stream);
/* t_v[k] = sum_s e_s[k] * (sum_r coef[(v * ns + s) * nr + r] * x_r[k]), r first, then s, both ascending:
 * the operations of emg3d_dev_sensitivity_combine term by term, so row v of t is bit-identical to its
 * result with the coefficients coef + v * ns * nr. t: nv rows of n elements of the fields' type, WRITTEN,
 * row v starts v * t_stride elements behind row 0, t_stride >= n (what lies between the rows is not
 * touched). coef: device, nv * ns * nr elements. One thread per k keeps its receiver values and loads
 * every e_s[k] once for up to 8 vectors; more vectors: one pass over the stacks per 8 (nv = 1 runs the
 * kernel of emg3d_dev_sensitivity_combine). */
int emg3d_dev_sensitivity_combine_block(size_t n, int is_complex, const void *e, size_t e_stride, int ns,
                                        const void *x, size_t x_stride, int nr, const void *coef, int nv,
                                        void *t, size_t t_stride, void *stream);
/* The two for stacks stored in single precision (conventions of the _sp entry points above): NARROW e, x;
 * fp64: w, scale, out, ws, coef, t. 16-byte loads where every row of both stacks and of w (of t) starts on
 * a 16-byte boundary, element-wise loads otherwise; t does not depend on which are used. */
int emg3d_dev_sensitivity_dots_block_sp(size_t n, int is_complex, const void *e, size_t e_stride, int ns,
                                        const void *x, size_t x_stride, int nr, const double *w,
                                        size_t w_stride, int nv, double scale_re, double scale_im,
                                        void *out, double *ws, size_t ws_len, void *stream);
int emg3d_dev_sensitivity_combine_block_sp(size_t n, int is_complex, const void *e, size_t e_stride,
                                           int ns, const void *x, size_t x_stride, int nr,
                                           const void *coef, int nv, void *t, size_t t_stride,
                                           void *stream);

/* ---- the inner solve of a Gauss-Newton step: regulariser and block PCG -----------
 * (R v)[c] = a[c] (alpha_s V_c v[c] + sum_{d} alpha_d sum_{faces f of c along d} a[c'] A_f / l_f (v[c] - v[c'])) on a
 * tensor grid of nx x ny x nz cells, x fastest: V_c cell volume, A_f face area, l_f half the sum of the two widths
 * along d, a = mask (device, one byte per cell, 0 / 1; NULL: all active). Faces on the boundary and towards an
 * inactive cell are left out, rows of inactive cells are 0. hx / hy / hz: device cell widths. The coefficients are
 * formed in the kernel from the widths, once per cell for all vectors, and never stored (csrc/regularise.h).
 *
 * emg3d_dev_model_regulariser: q[j] = beta q[j] + lam[j / vec_per_col] (R p[j]) for j < nvec; vector j starts
 * j * nx ny nz doubles behind vector 0 (the device blocks of the block products with vec_per_col components per
 * column); nvec a multiple of vec_per_col; beta = 0: q is written, not read; lam: device, nvec / vec_per_col
 * doubles, NULL: 1; p and q must not overlap. pq not NULL: pq[col] = sum over the column's vec_per_col vectors of
 * <p, q_new> (device, written), from the same pass. No floating-point atomics: every wave of 64 cells (a row piece
 * of the (64, 4, 1) workgroup) adds its share with shuffles and writes one partial sum, ws[col * nwaves + wave]
 * with wave = 4 * (bx + nbx (by + nby iz)) + row piece; a second launch adds the partials of a column, thread t of
 * 256 taking t, t + 256, ... in ascending order, then a binary tree over the threads. The order depends on the sizes
 * alone: the same call gives the same bits. ws: at least emg3d_model_regulariser_ws_len doubles (0: bad sizes),
 * needed only with pq. A direction may have 1 or 2 cells. nx ny nz < 2^31. */
size_t emg3d_model_regulariser_ws_len(int nx, int ny, int nz, int nvec, int vec_per_col);
int emg3d_dev_model_regulariser(int nx, int ny, int nz, const double *hx, const double *hy, const double *hz,
                                double alpha_s, double alpha_x, double alpha_y, double alpha_z,
                                const unsigned char *mask, int nvec, int vec_per_col, const double *p, double *q,
                                double beta, const double *lam, double *pq, double *ws, size_t ws_len,
                                void *stream);
/* diag[c] = (R)_cc: a[c] (alpha_s V_c + sum of the coefficients of the faces that R keeps); nx ny nz doubles. */
int emg3d_dev_model_regulariser_diagonal(int nx, int ny, int nz, const double *hx, const double *hy,
                                         const double *hz, double alpha_s, double alpha_x, double alpha_y,
                                         double alpha_z, const unsigned char *mask, double *diag, void *stream);
/* The weighted / sparse-norm (IRLS, lagged diffusivity) form of R. Component k < vec_per_col <= 3 of
 * a column has cell weights w_k >= 0 and linearisation values u_k, both shared by all columns:
 *   cs[c]   = alpha_s V_c w[c] rho(p_s, eps_s; u[c])
 *   cf[c,f] = alpha_d a[c'] (A_f / l_f) (w[c] + w[c']) / 2 rho(p_d, eps_g; (u[c] - u[c']) / l_f)
 *   rho(p, eps; t) = (t^2 + eps^2)^(p / 2 - 1), exactly 1 (nothing read, nothing multiplied) for p = 2
 * in (R v)[c] = a[c] (cs[c] v[c] + sum_f cf[c,f] (v[c] - v[c'])); everything else as emg3d_dev_model_regulariser. Each
 * factor of a face is the same from either side: R is symmetric as stored, positive semi-definite, and annihilates
 * constants when alpha_s = 0. cell_weights: device, row k starts k * weights_stride doubles behind row 0 (stride 0: one
 * row of nx ny nz doubles for all components), NULL: 1. linearise_at: device, rows as for the weights by
 * linearise_stride; NULL only if all four norms are 2 (then it and the thresholds are not used). The norms p_s, p_x,
 * p_y, p_z lie in [0, 2]; p = 1 takes a reciprocal square root, p = 0 a reciprocal, every other the power function.
 * The coefficients of all components are formed in registers once per cell (w and u of the neighbours through the
 * cache, a face that R leaves out reads the cell itself) and serve all columns; then the loop, the order of the
 * additions, the partial sums of <p, q_new> in ws and the second launch are those of emg3d_dev_model_regulariser
 * (ws: emg3d_model_regulariser_ws_len). With cell_weights NULL or all 1.0 and all norms 2 the bits are those of
 * emg3d_dev_model_regulariser. EMG3D_ERR_BADARG, nothing launched: vec_per_col > 3, nvec not a multiple of it, a norm
 * outside [0, 2] or not finite, a norm != 2 with linearise_at NULL or with eps_s or eps_g not finite and > 0, a stride
 * that is neither 0 nor >= nx ny nz, and what emg3d_dev_model_regulariser refuses. */
int emg3d_dev_model_regulariser_weighted(int nx, int ny, int nz, const double *hx, const double *hy, const double *hz,
                                         double alpha_s, double alpha_x, double alpha_y, double alpha_z,
                                         const unsigned char *mask, const double *cell_weights, size_t weights_stride,
                                         const double *linearise_at, size_t linearise_stride, double p_s, double p_x,
                                         double p_y, double p_z, double eps_s, double eps_g, int nvec, int vec_per_col,
                                         const double *p, double *q, double beta, const double *lam, double *pq,
                                         double *ws, size_t ws_len, void *stream);
/* diag[k * nx ny nz + c] = (R_k)_cc of the weighted operator of component k < vec_per_col: vec_per_col x nx ny nz
 * doubles, 0 on inactive cells. With weights NULL or 1.0 and all norms 2: the bits of
 * emg3d_dev_model_regulariser_diagonal in every row. */
int emg3d_dev_model_regulariser_weighted_diagonal(int nx, int ny, int nz, const double *hx, const double *hy,
                                                  const double *hz, double alpha_s, double alpha_x, double alpha_y,
                                                  double alpha_z, const unsigned char *mask, const double *cell_weights,
                                                  size_t weights_stride, const double *linearise_at,
                                                  size_t linearise_stride, double p_s, double p_x, double p_y,
                                                  double p_z, double eps_s, double eps_g, int vec_per_col, double *diag,
                                                  void *stream);
/* Block preconditioned CG: ncol independent systems whose vectors are the columns (vec_per_col x n_cells doubles
 * each, contiguous) of x, r, p, q. The scalars live in `table` (device), 8 doubles per column:
 *   [0] lambda  [1] <b,b>  [2] <r,z>  [3] <r,z> before  [4] <p,q>  [5] <r,r>  [6] iterations  [7] state
 * state 0 running, 1 converged (<r,r> <= tol^2 <b,b>), 2 breakdown (<p,q> <= 0, or <r,z> <= 0 with r != 0), 3 a sum is not finite. The host
 * writes lambda and zeros; a column whose state is not 0 is FROZEN: no kernel below touches its x, r, p again.
 * Preconditioner z = M r: r / (hdiag + lambda rdiag) (hdiag: vec_per_col x n_cells, shared by the columns; rdiag:
 * n_cells; both device; where the sum is not > 0: r), r itself with hdiag NULL, and 0 where mask is 0.
 *
 * emg3d_dev_pcg_update, per running column: alpha = <r,z> / pq[col], x += alpha p, r -= alpha q (0 where mask is 0),
 * and the partial sums of <r, z> and <r, r> with the new r into ws (per workgroup; at least emg3d_pcg_ws_len
 * doubles). pq[col] not in (0, inf]: the column is left as it is. first != 0: the set-up, r (holding b) is masked
 * and summed, x / p / q / pq are not used.
 * emg3d_dev_pcg_scalar: one workgroup adds the partial sums of emg3d_dev_pcg_update in a fixed order (thread t of
 * 256: t, t + 256, ..., then a binary tree) and advances the table: pq[col] <= 0 or NaN -> state 2 / 3; otherwise
 * <r,z> -> [3], the sums -> [2], [5], iterations + 1, and the new state. first != 0: [1] = [5] = <b,b>, state 1 if
 * that is 0.
 * emg3d_dev_pcg_direction, per running column: p = z + ([2] / [3]) p with z = M r formed again from r (first: p = z). */
size_t emg3d_pcg_table_len(int ncol);
size_t emg3d_pcg_ws_len(size_t n_cells, int ncol);
int emg3d_dev_pcg_update(size_t n_cells, int vec_per_col, int ncol, int first, double *x, double *r, const double *p,
                         const double *q, const double *hdiag, const double *rdiag, const unsigned char *mask,
                         const double *table, const double *pq, double *ws, size_t ws_len, void *stream);
int emg3d_dev_pcg_scalar(size_t n_cells, int ncol, int first, double tol, double *table, const double *pq,
                         const double *ws, size_t ws_len, void *stream);
int emg3d_dev_pcg_direction(size_t n_cells, int vec_per_col, int ncol, int first, double *p, const double *r,
                            const double *hdiag, const double *rdiag, const unsigned char *mask,
                            const double *table, void *stream);
/* emg3d_dev_pcg_update / emg3d_dev_pcg_direction with one diagonal of R per component: component k reads
 * rdiag[k * rdiag_stride + c]. rdiag_stride 0: one row for all components (the two entries above, which forward
 * here with 0: the same kernels, the same bits); otherwise >= n_cells and rdiag holds vec_per_col rows
 * (emg3d_dev_model_regulariser_weighted_diagonal). It changes only an address. */
int emg3d_dev_pcg_update_rd(size_t n_cells, int vec_per_col, int ncol, int first, double *x, double *r, const double *p,
                            const double *q, const double *hdiag, const double *rdiag, size_t rdiag_stride,
                            const unsigned char *mask, const double *table, const double *pq, double *ws,
                            size_t ws_len, void *stream);
int emg3d_dev_pcg_direction_rd(size_t n_cells, int vec_per_col, int ncol, int first, double *p, const double *r,
                               const double *hdiag, const double *rdiag, size_t rdiag_stride,
                               const unsigned char *mask, const double *table, void *stream);
/* emg3d_dev_pcg_update / emg3d_dev_pcg_direction with the block-Jacobi preconditioner: per cell c
 * z_c = (B_c + lambda diag(rd_c))^-1 r_c, B_c the symmetric vec_per_col x vec_per_col block of the packed rows of
 * emg3d_dev_hessian_cell_blocks (hblocks, rows hblocks_stride >= n_cells apart, already times the chain factors), rd
 * as for the _rd entries. vec_per_col in {2, 3}: 1 is refused, the entries above serve it. A thread takes a cell and
 * all its components, factorises by Cholesky in registers and solves; where a pivot is not finite and > 0 the cell
 * falls back to the Jacobi rule of the entries above on the diagonal rows, component by component. Everything else
 * -- alpha, beta, frozen columns, masks, the layout of ws -- as there; emg3d_dev_pcg_scalar follows unchanged.
 * EMG3D_ERR_BADARG, nothing launched: hblocks or rdiag NULL, a stride below n_cells (rdiag_stride may be 0). */
int emg3d_dev_pcg_update_blk(size_t n_cells, int vec_per_col, int ncol, int first, double *x, double *r, const double *p,
                             const double *q, const double *hblocks, size_t hblocks_stride, const double *rdiag,
                             size_t rdiag_stride, const unsigned char *mask, const double *table, const double *pq,
                             double *ws, size_t ws_len, void *stream);
int emg3d_dev_pcg_direction_blk(size_t n_cells, int vec_per_col, int ncol, int first, double *p, const double *r,
                                const double *hblocks, size_t hblocks_stride, const double *rdiag, size_t rdiag_stride,
                                const unsigned char *mask, const double *table, void *stream);
/* The data-space (Woodbury) preconditioner of the block PCG above: with dinv = 1 / diag R (1 where
 * that is not positive, 0 on inactive cells; vec_per_col rows dinv_stride doubles apart, stride 0: one row for all
 * components), s = sqrt(data weights) and the eigenpairs (Q, L) of diag(s) J^ diag(dinv) J^T diag(s), per running column
 *   u = dinv o r / lambda,   y = diag(s) Q diag(lambda / (lambda + L)) Q^T diag(s) (J^ u),   z = u - dinv o (J^T y) / lambda
 * is z = (lambda diag R + J^T diag(s) Q Q^T diag(s) J^)^-1 r exactly, for every number of eigenpairs kept. J^ u and
 * J^T y are a block pass over the kept fields (emg3d_dev_sensitivity_dots_block / _combine_block); the entries below
 * are the rest. All fp64, no floating-point atomics, every sum in an order fixed by the sizes: same call, same bits.
 * A column runs if its state [7] is 0 and (first != 0 or pq[col] in (0, inf]), as for emg3d_dev_pcg_update; the
 * vector entries leave every element of another column as it is.
 *
 * emg3d_dev_pcg_scale: u = dinv o r / [0] per running column.
 * emg3d_dev_data_space_filter: y (ncol x n_data) from d (ncol x n_data), both device, rows contiguous. q: n_data x rank
 * doubles, row-major (the eigenvector of eigenvalues[j] >= 0 is column j), rank <= n_data; s: n_data. Two launches per
 * eight columns, t = diag(phi) Q^T (s o d) into ws (emg3d_data_space_filter_ws_len doubles) and y = s o (Q t): Q is
 * read once per stage for eight columns. A column whose state is not 0 gets y = 0, written.
 * emg3d_dev_pcg_finish: z = u - dinv o g / [0] per running column, 0 where mask is 0, and the partial sums of <r, z>
 * and <r, r> into ws in the layout of emg3d_dev_pcg_update (emg3d_pcg_ws_len doubles): emg3d_dev_pcg_scalar follows
 * unchanged. Columns that do not run contribute zeros there, which emg3d_dev_pcg_scalar does not read.
 * emg3d_dev_pcg_direction_z, per column of state 0: p = z + ([2] / [3]) p from the stored z (first: p = z).
 * EMG3D_ERR_BADARG, nothing launched: sizes < 1, ncol > 65535 (vector entries), rank > n_data, a NULL or aliased
 * vector, a stride that is neither 0 nor >= n_cells, pq NULL with first == 0; EMG3D_ERR_SCRATCH: ws too small. */
int emg3d_dev_pcg_scale(size_t n_cells, int vec_per_col, int ncol, int first, double *u, const double *r,
                        const double *dinv, size_t dinv_stride, const double *table, const double *pq, void *stream);
size_t emg3d_data_space_filter_ws_len(int rank, int ncol);
int emg3d_dev_data_space_filter(int n_data, int rank, int ncol, const double *q, const double *eigenvalues,
                                const double *s, const double *d, double *y, const double *table, double *ws,
                                size_t ws_len, void *stream);
int emg3d_dev_pcg_finish(size_t n_cells, int vec_per_col, int ncol, int first, double *z, const double *u,
                         const double *g, const double *r, const double *dinv, size_t dinv_stride,
                         const unsigned char *mask, const double *table, const double *pq, double *ws, size_t ws_len,
                         void *stream);
int emg3d_dev_pcg_direction_z(size_t n_cells, int vec_per_col, int ncol, int first, double *p, const double *z,
                              const double *table, void *stream);
/* The two primitives of subspace methods on device blocks (randomised SVD, block Lanczos, Nystroem).
 * A block is ncol rows of n doubles, `stride` doubles apart (the model blocks of the block products: n = components
 * x cells). All fp64, no atomics, every sum in an order fixed by the sizes: same call, same bits. Nothing behind n
 * is read in any row.
 *
 * emg3d_dev_block_gram: g[i * ncol + j] = sum_k y_i[k] y_j[k], ncol x ncol device doubles, symmetric bit for bit
 * (i <= j is computed, [j, i] is its copy). Two stages: a partial per entry and chunk of 4096 elements into ws (at
 * least emg3d_block_gram_ws_len(n, ncol) = ncol^2 ceil(n / 4096) doubles; 0 for sizes that are refused), then one
 * workgroup per entry adds them (thread t of 256: t, t + 256, ..., then a binary tree).
 * emg3d_dev_block_rotate: out_j[k] = sum_i y_i[k] t[i * ncol_out + j], the sum over i ascending; t: ncol_in x
 * ncol_out device doubles, row-major. Out of place; nothing between the rows of out is written.
 * EMG3D_ERR_BADARG, nothing launched: a NULL pointer, n < 1, ncol outside 1..64 (rotate: not 1 <= ncol_out <=
 * ncol_in <= 64), a stride smaller than n, y and out overlapping. */
size_t emg3d_block_gram_ws_len(size_t n, int ncol);
int emg3d_dev_block_gram(size_t n, int ncol, const double *y, size_t stride, double *g, double *ws, void *stream);
int emg3d_dev_block_rotate(size_t n, int ncol_in, int ncol_out, const double *y, size_t stride, const double *t,
                           double *out, size_t out_stride, void *stream);

/* ---- before a solve: model re-gridding -------------------------------
 * maps.interp_volume_average (emg3d/maps.py:555-616) behind Model.interpolate_to_grid
 * (emg3d/models.py:322-366). values (nx,ny,nz) -> out (mx,my,mz), doubles, x fastest. Per axis
 * the host supplies maps._volume_average_weights (maps.py:619-664) grouped by output cell:
 * seg* (m+1 offsets), w* (segment lengths), in* (input cell of each segment); new_vol = output
 * cell volumes. Same additions in the same order as the reference: bit-identical. log10_scale = 1:
 * the values are averaged on a log10 scale (maps.interpolate(log=True), emg3d/maps.py:346-358).
 * log10_scale = 2: the ADJOINT of the linear averaging (maps._interp_volume_average_adj,
 * emg3d/maps.py:722-750 -- the gradient's way back from a computational grid): the tables are the
 * transposed ones (grouped by ORIGINAL cell = output cell of this call), `values` and `new_vol`
 * both live on the averaged grid (nx,ny,nz), and out (mx,my,mz) is ACCUMULATED:
 * out_i += sum_o overlap_io / new_vol_o * values_o. */
int emg3d_dev_volume_average(const double *values, int nx, int ny, int nz, const int32_t *segx,
                             const int32_t *segy, const int32_t *segz, const double *wx,
                             const double *wy, const double *wz, const int32_t *inx,
                             const int32_t *iny, const int32_t *inz, const double *new_vol, int mx,
                             int my, int mz, double *out, int log10_scale, void *stream);

/* fields.get_source_field -> _dipole_vector (emg3d/fields.py:386-519, 792-938): the source vector
 * of a dipole / wire through `npoints` points (device, npoints x 3, metres), times the complex
 * factor `scale` (strength x (-s mu0)), ADDED to sx|sy|sz with atomic adds -- one thread walks one
 * straight segment from grid plane to grid plane. nodes_* (n + 1) and h* (n): device doubles. */
int emg3d_dev_source_field(int nx, int ny, int nz, int is_complex, const double *nodes_x, const double *nodes_y,
                           const double *nodes_z, const double *hx, const double *hy, const double *hz,
                           const double *points, int npoints, double scale_re, double scale_im, void *sx,
                           void *sy, void *sz, void *stream);

/* models.VolumeModel (emg3d/models.py:654-691) on the device: eta_{x,y,z} = -s mu0 V (sigma [+ s eps0
 * eps_r]) and zeta = V / mu_r from the model's PROPERTY arrays (nx,ny,nz doubles; property_y /
 * property_z / epsilon_r / mu_r may be NULL) and its mapping (0 Conductivity, 1 Resistivity,
 * 2 LgConductivity, 3 LgResistivity, 4 LnConductivity, 5 LnResistivity; emg3d/maps.py:120-330);
 * hx/hy/hz: cell widths (device); s mu0 and s eps0 as (re, im) (real fields: re only). eta_y / eta_z
 * are written only when property_y / property_z are given -- the caller aliases them to eta_x
 * otherwise, as the reference does (emg3d/models.py:693-712). */
int emg3d_dev_volume_model(int nx, int ny, int nz, int is_complex, const double *property_x,
                           const double *property_y, const double *property_z, const double *epsilon_r,
                           const double *mu_r, int mapping, const double *hx, const double *hy,
                           const double *hz, double smu0_re, double smu0_im, double seps0_re,
                           double seps0_im, void *eta_x, void *eta_y, void *eta_z, double *zeta,
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EMG3D_AMD_H */
