// Data-space Gauss-Newton matrix from the kept fields of reciprocal.h: one block of
//     G = J^ diag(m) J^T,   rows of J^: Re J_i (first half), Im J_i (second half; complex fields only),
// between the data of a side A and a side B (two frequencies, or one and the same). With hessian.h's pair sums Z,
//     a^_{i,p}(c) = Re | Im ( scale_A sum_{d: row[d] = p} Z^A_{s,r,d}(c) ),       i = s nr + r,
//     out[i, j] = sum_{p, c} mw[p, c] (V_c / 4)^2 a^_{i,p}(c) b^_{j,p}(c) :
// a SYRK whose operand is generated on the fly and never written to memory.
// A workgroup owns one pair of output tiles -- a tile is GR_TS sources x GR_TR receivers = 32 data of a side, R = 32
// (real fields) or 64 (complex: Re and Im) rows -- and grid-strides over patches of GR_PX x GR_PY x GR_PZ = 64 cells.
// Per patch and property row p:
//   1. panels. Per direction of the row the edges of the patch (with the upper halo) of the tile's 4 + 8 fields are
//      staged in LDS; thread (cell, q) adds the four edges of its cell into the pair sums of the 4 sources and the
//      receivers 2q, 2q + 1 of the tile (registers), scales them and writes f a^ with f = sqrt(mw) V / 4 into the
//      side's panel [cell][row] in LDS. BOTH sides carry f, so a diagonal tile of a symmetric block needs one panel.
//   2. rank update. Wave w takes the cells 16 w .. 16 w + 15 of the panel: lane (li, lj) adds a[li-th R/8 rows] x
//      b[lj-th R/8 rows] into an R/8 x R/8 register block (8 x 8 for complex fields) that lives across all patches.
// At the end the four waves' blocks are added through LDS in wave order and the tile goes to `ws`; a second launch
// adds the workgroups' partial tiles in ascending order, scatters them to `out` and, for a symmetric block (the same
// stacks and scales on both sides), takes every entry below the diagonal from its mirror image: only the tile pairs
// ta <= tb are computed then. Plain fp64, no atomics; the order of every sum depends on the sizes alone.
// Fields of a ragged tile and edges outside the grid are not read (zeros in LDS), cells outside the grid have f = 0.
// Included at the end of kernels.hip (one translation unit), after hessian.h.
#pragma once

namespace {

constexpr int GR_PX = 16, GR_PY = 2, GR_PZ = 2;              // the patch; GR_PX complex values = 256 B per row
constexpr int GR_CELLS = GR_PX * GR_PY * GR_PZ;
constexpr int GR_THREADS = 256, GR_WAVES = GR_THREADS / 64;
constexpr int GR_TS = 4, GR_TR = 8;                          // the tile of a side: 32 data
constexpr int GR_DATA = GR_TS * GR_TR;
constexpr int GR_FIELDS = GR_TS + GR_TR;
constexpr int GR_EDGES = GR_PX * (GR_PY + 1) * (GR_PZ + 1); // x-edges of a patch, the most of the three directions
constexpr int GR_MAX_WG = 256;                               // workgroups per tile pair: one per compute unit
static_assert((GR_PX + 1) * GR_PY * (GR_PZ + 1) <= GR_EDGES && (GR_PX + 1) * (GR_PY + 1) * GR_PZ <= GR_EDGES, "LDS tile");
static_assert(GR_CELLS == 64 && GR_THREADS == 4 * GR_CELLS && GR_TR == 2 * (GR_THREADS / GR_CELLS), "thread = (cell, q)");
static_assert(GR_CELLS % GR_WAVES == 0 && GR_DATA == 32, "a wave's share of the panel; eight lanes of R / 8 rows");

template <class T> struct GramRows { static constexpr int R = GR_DATA * (int)(sizeof(T) / sizeof(double)), PS = R + 2; };
// staging + two panels of PS = R + 2 doubles per cell (the padding spreads a wave's panel writes over the banks);
// the waves' final sum (R x R) reuses the panels
// S: the type the stacks are stored in (T, or its single-precision partner). The edges are staged AS STORED and widened
// when a thread reads them for its pair sums; the panels and everything behind them are fp64 whatever S is.
template <class T, class S = T> constexpr size_t gram_lds_bytes()
{
    return (size_t)GR_FIELDS * GR_EDGES * sizeof(S) + (size_t)2 * GR_CELLS * GramRows<T>::PS * sizeof(double);
}
static_assert((size_t)GR_FIELDS * GR_EDGES * sizeof(float) % 16 == 0, "the panels start on a 16-byte boundary behind any stage");
static_assert((size_t)GramRows<cplx>::R * GramRows<cplx>::R <= (size_t)2 * GR_CELLS * GramRows<cplx>::PS, "final sum in the panels");
static_assert((size_t)GramRows<double>::R * GramRows<double>::R <= (size_t)2 * GR_CELLS * GramRows<double>::PS, "final sum in the panels");
static_assert(gram_lds_bytes<cplx>() <= (size_t)160 * 1024, "LDS of a compute unit");

template <class T, class S> struct GramSide {
    const S *e;
    size_t es;
    int ns;
    const S *x;
    size_t xs;
    int nr;
    T scale;
    int ntr;                                                 // receiver tiles: tile t = (t / ntr, t % ntr)
};

__device__ __forceinline__ double gram_re(cplx a) { return a.re; }
__device__ __forceinline__ double gram_re(double a) { return a; }
__device__ __forceinline__ double gram_im(cplx a) { return a.im; }
__device__ __forceinline__ double gram_im(double) { return 0.0; }

// Step 1 for one side: the panel rows of tile `tile` for the patch at (x0, y0, z0) and property row p.
template <class T, class S>
__device__ __forceinline__ void gram_panel(int nx, int ny, int nz, const GramSide<T, S> &A, int tile, int x0, int y0, int z0,
                                           int p, int row_x, int row_y, int row_z, double f, S *__restrict__ stage,
                                           double *__restrict__ panel)
{
    constexpr int PS = GramRows<T>::PS;
    const int t = threadIdx.x;
    const int tx = t % GR_PX, trow = t / GR_PX;             // staging: thread tx of row slot trow
    const int cl = t % GR_CELLS, q = t / GR_CELLS;          // the thread's cell in the patch and its receiver pair
    const int cx = cl % GR_PX, cy = (cl / GR_PX) % GR_PY, cz = cl / (GR_PX * GR_PY);
    const int s0 = (tile / A.ntr) * GR_TS, r0 = (tile % A.ntr) * GR_TR;
    const size_t n_x = (size_t)nx * (ny + 1) * (nz + 1), n_y = (size_t)(nx + 1) * ny * (nz + 1);
    T acc[GR_TS][2];
#pragma unroll
    for (int i = 0; i < GR_TS; ++i) acc[i][0] = acc[i][1] = emg::zero<T>();
#pragma unroll 1
    for (int d = 0; d < 3; ++d) {
        if ((d == 0 ? row_x : d == 1 ? row_y : row_z) != p) continue;
        // the d-edges: (gnx, gny, gnz) of them on the grid, (lx, ly, lz) on the patch
        const int gnx = nx + (d != 0), gny = ny + (d != 1), gnz = nz + (d != 2);
        const int lx = GR_PX + (d != 0), ly = GR_PY + (d != 1), lz = GR_PZ + (d != 2);
        const size_t goff = d == 0 ? 0 : d == 1 ? n_x : n_x + n_y;
        const int nrows = ly * lz;
        __syncthreads();                                    // the previous stage and the panels have been used up
        for (int idx = trow; idx < GR_FIELDS * nrows; idx += GR_THREADS / GR_PX) {
            const int fld = idx / nrows, row = idx % nrows;
            const int gj = y0 + row % ly, gk = z0 + row / ly;
            const bool have = fld < GR_TS ? s0 + fld < A.ns : r0 + (fld - GR_TS) < A.nr;
            const S *const src = !have ? A.e : fld < GR_TS ? A.e + (size_t)(s0 + fld) * A.es
                                                             : A.x + (size_t)(r0 + (fld - GR_TS)) * A.xs;
            for (int li = tx; li < lx; li += GR_PX) {
                const int gi = x0 + li;
                const bool in = have && gi < gnx && gj < gny && gk < gnz;
                const size_t g = goff + gi + (size_t)gnx * (gj + (size_t)gny * gk);
                stage[fld * GR_EDGES + li + lx * row] = in ? src[g] : emg::narrow<S>(emg::zero<T>());
            }
        }
        __syncthreads();
        // the four d-edges of the cell in the order of edges_to_cell: x: y inner, z outer; y: x, z; z: x, y
        const int o1 = d == 0 ? lx : 1, o2 = d == 2 ? lx : lx * ly;
        const S *const src = stage + (cx + lx * (cy + ly * cz));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const S *const e4 = src + ((k & 1) * o1 + (k >> 1) * o2);
            const T x0v = emg::widen(e4[(GR_TS + 2 * q) * GR_EDGES]), x1v = emg::widen(e4[(GR_TS + 2 * q + 1) * GR_EDGES]);
#pragma unroll
            for (int i = 0; i < GR_TS; ++i) {
                const T ev = emg::widen(e4[i * GR_EDGES]);
                acc[i][0] = emg::mad(ev, x0v, acc[i][0]);
                acc[i][1] = emg::mad(ev, x1v, acc[i][1]);
            }
        }
    }
    double *const dst = panel + cl * PS + 2 * q;
#pragma unroll
    for (int i = 0; i < GR_TS; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const T v = A.scale * acc[i][j];
            dst[i * GR_TR + j] = f * gram_re(v);
            if (sizeof(T) > sizeof(double)) dst[GR_DATA + i * GR_TR + j] = f * gram_im(v);
        }
}

template <class T, class S>
__global__ __launch_bounds__(GR_THREADS) void k_data_gram(int nx, int ny, int nz, GramSide<T, S> A, GramSide<T, S> B, int n_tiles_b,
                                                          int same, int row_x, int row_y, int row_z,
                                                          const double *__restrict__ mw, size_t mws,
                                                          const double *__restrict__ vol, int npx, int npy, int n_patches,
                                                          double *__restrict__ ws)
{
    constexpr int R = GramRows<T>::R, PS = GramRows<T>::PS, RB = R / 8;
    extern __shared__ double2 gr_smem[];
    S *const stage = reinterpret_cast<S *>(gr_smem);                          // [GR_FIELDS][GR_EDGES]
    double *const panel_a = reinterpret_cast<double *>(stage + GR_FIELDS * GR_EDGES);   // [GR_CELLS][PS]
    double *const panel_b = panel_a + GR_CELLS * PS;
    const int ta = blockIdx.y / n_tiles_b, tb = blockIdx.y % n_tiles_b;
    if (same && ta > tb) return;                            // the mirror image of (tb, ta): the second launch copies it
    const bool one_panel = same && ta == tb;
    const int t = threadIdx.x;
    const int cl = t % GR_CELLS, wave = t / 64;
    const int cx = cl % GR_PX, cy = (cl / GR_PX) % GR_PY, cz = cl / (GR_PX * GR_PY);
    const int li = (t % 64) % 8, lj = (t % 64) / 8;         // rank update: rows li RB .. of A by rows lj RB .. of B
    double acc[RB][RB];
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < RB; ++j) acc[i][j] = 0.0;

#pragma unroll 1
    for (int patch = blockIdx.x; patch < n_patches; patch += gridDim.x) {
        const int x0 = (patch % npx) * GR_PX, y0 = ((patch / npx) % npy) * GR_PY, z0 = (patch / (npx * npy)) * GR_PZ;
        const int ix = x0 + cx, iy = y0 + cy, iz = z0 + cz;
        const bool inside = ix < nx && iy < ny && iz < nz;
        const size_t c = inside ? (size_t)ix + (size_t)nx * (iy + (size_t)ny * iz) : 0;
        const double q4 = inside ? vol[c] / 4 : 0.0;
#pragma unroll 1
        for (int p = 0; p < 3; ++p) {
            if (row_x != p && row_y != p && row_z != p) continue;
            const double f = inside ? sqrt(mw[p * mws + c]) * q4 : 0.0;
            gram_panel<T, S>(nx, ny, nz, A, ta, x0, y0, z0, p, row_x, row_y, row_z, f, stage, panel_a);
            if (!one_panel) gram_panel<T, S>(nx, ny, nz, B, tb, x0, y0, z0, p, row_x, row_y, row_z, f, stage, panel_b);
            __syncthreads();
            const double *pa = panel_a + (wave * (GR_CELLS / GR_WAVES)) * PS + li * RB;
            const double *pb = (one_panel ? panel_a : panel_b) + (wave * (GR_CELLS / GR_WAVES)) * PS + lj * RB;
#pragma unroll 2
            for (int k = 0; k < GR_CELLS / GR_WAVES; ++k) {
                double a[RB], b[RB];
#pragma unroll
                for (int i = 0; i < RB; ++i) a[i] = pa[k * PS + i];
#pragma unroll
                for (int j = 0; j < RB; ++j) b[j] = pb[k * PS + j];
#pragma unroll
                for (int i = 0; i < RB; ++i)
#pragma unroll
                    for (int j = 0; j < RB; ++j) acc[i][j] = __builtin_fma(a[i], b[j], acc[i][j]);
            }
        }
    }
    // the four waves' blocks, added in wave order, then the tile to this workgroup's place in ws
    double *const red = panel_a;
#pragma unroll 1
    for (int w = 0; w < GR_WAVES; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    double *const r = red + (li * RB + i) * R + (lj * RB + j);
                    *r = w == 0 ? acc[i][j] : *r + acc[i][j];
                }
        }
    }
    __syncthreads();
    double *const part = ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (R * R);
    for (int i = t; i < R * R; i += GR_THREADS) part[i] = red[i];
}

// Second launch: out[i, j] = sum over the workgroups g (ascending) of their partial tiles; a symmetric block takes the
// entries below the diagonal from their mirror images.
__global__ __launch_bounds__(256) void k_data_gram_reduce(int c, int ns_a, int nr_a, int ntr_a, int ns_b, int nr_b, int ntr_b,
                                                          int n_tiles_b, int same, int n_wg, const double *__restrict__ ws,
                                                          double *__restrict__ out, size_t ld)
{
    const int n_a = ns_a * nr_a, n_b = ns_b * nr_b, R = GR_DATA * c;
    const int j = blockIdx.x * 16 + threadIdx.x % 16, i = blockIdx.y * 16 + threadIdx.x / 16;
    if (i >= c * n_a || j >= c * n_b) return;
    const int sa = (i % n_a) / nr_a, ra = (i % n_a) % nr_a, sb = (j % n_b) / nr_b, rb = (j % n_b) % nr_b;
    int ta = (sa / GR_TS) * ntr_a + ra / GR_TR, la = (i / n_a) * GR_DATA + (sa % GR_TS) * GR_TR + ra % GR_TR;
    int tb = (sb / GR_TS) * ntr_b + rb / GR_TR, lb = (j / n_b) * GR_DATA + (sb % GR_TS) * GR_TR + rb % GR_TR;
    if (same && (ta > tb || (ta == tb && la > lb))) {
        int h = ta; ta = tb; tb = h;
        h = la; la = lb; lb = h;
    }
    const double *src = ws + (size_t)(ta * n_tiles_b + tb) * n_wg * (R * R) + la * R + lb;
    double sum = 0.0;
    for (int g = 0; g < n_wg; ++g) sum += src[(size_t)g * (R * R)];
    out[(size_t)i * ld + j] = sum;
}

inline size_t gram_patches(int nx, int ny, int nz)
{
    return (size_t)cdiv(nx, GR_PX) * cdiv(ny, GR_PY) * cdiv(nz, GR_PZ);
}

// Doubles of workspace: one partial tile per workgroup -- min(patches, GR_MAX_WG) workgroups for each pair of tiles
// when the tiles are full, and at least one for every pair of tiles of the most ragged split of n = ns nr data
// (cdiv(ns, 4) cdiv(nr, 8) <= cdiv(n, 4)).
inline size_t gram_ws_len(int nx, int ny, int nz, int is_complex, int n_a, int n_b)
{
    const size_t R = (size_t)GR_DATA * (is_complex ? 2 : 1);
    const size_t wg = std::min(gram_patches(nx, ny, nz), (size_t)GR_MAX_WG);
    const size_t full = wg * cdiv(n_a, GR_DATA) * cdiv(n_b, GR_DATA), ragged = (size_t)cdiv(n_a, 4) * cdiv(n_b, 4);
    return R * R * std::max(full, ragged);
}

template <class T> T gram_scale(double re, double im);
template <> inline double gram_scale<double>(double re, double) { return re; }
template <> inline cplx gram_scale<cplx>(double re, double im) { return cplx(re, im); }

template <class T, class S>
int launch_data_gram(int nx, int ny, int nz, const GramSide<T, S> &A, const GramSide<T, S> &B, int n_tiles_a, int n_tiles_b, int same,
                     int n_wg, int row_x, int row_y, int row_z, const double *mw, size_t mws, const double *vol, double *out,
                     size_t ld, double *ws, hipStream_t st)
{
    constexpr size_t smem = gram_lds_bytes<T, S>();
    constexpr int c = (int)(sizeof(T) / sizeof(double));
    if (smem > (size_t)64 * 1024) HIP_TRY(allow_lds((const void *)&k_data_gram<T, S>, smem));
    hipLaunchKernelGGL((k_data_gram<T, S>), dim3(n_wg, n_tiles_a * n_tiles_b), dim3(GR_THREADS), smem, st, nx, ny, nz, A, B, n_tiles_b,
                       same, row_x, row_y, row_z, mw, mws, vol, cdiv(nx, GR_PX), cdiv(ny, GR_PY), (int)gram_patches(nx, ny, nz), ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_data_gram_reduce, dim3(cdiv(c * B.ns * B.nr, 16), cdiv(c * A.ns * A.nr, 16)), dim3(256), 0, st, c, A.ns,
                       A.nr, A.ntr, B.ns, B.nr, B.ntr, n_tiles_b, same, n_wg, ws, out, ld);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <class T, class S>
int data_gram(int nx, int ny, int nz, const void *e_a, size_t es_a, int ns_a, const void *x_a, size_t xs_a, int nr_a,
              double sa_re, double sa_im, const void *e_b, size_t es_b, int ns_b, const void *x_b, size_t xs_b, int nr_b,
              double sb_re, double sb_im, int n_wg, int row_x, int row_y, int row_z, const double *mw, size_t mws,
              const double *vol, double *out, size_t ld, double *ws, hipStream_t st)
{
    const GramSide<T, S> A{(const S *)e_a, es_a, ns_a, (const S *)x_a, xs_a, nr_a, gram_scale<T>(sa_re, sa_im), cdiv(nr_a, GR_TR)};
    const GramSide<T, S> B{(const S *)e_b, es_b, ns_b, (const S *)x_b, xs_b, nr_b, gram_scale<T>(sb_re, sb_im), cdiv(nr_b, GR_TR)};
    const int same = e_a == e_b && x_a == x_b && es_a == es_b && xs_a == xs_b && ns_a == ns_b && nr_a == nr_b &&
                     sa_re == sb_re && (sizeof(T) == sizeof(double) || sa_im == sb_im);
    return launch_data_gram<T, S>(nx, ny, nz, A, B, cdiv(ns_a, GR_TS) * A.ntr, cdiv(ns_b, GR_TS) * B.ntr, same, n_wg, row_x, row_y,
                               row_z, mw, mws, vol, out, ld, ws, st);
}

// The checks of emg3d_dev_data_gram and of its _sp sibling (SP: the stacks of BOTH sides in single precision).
template <bool SP>
int data_gram_checked(int nx, int ny, int nz, int is_complex, const void *e_a, size_t e_a_stride, int ns_a, const void *x_a,
                      size_t x_a_stride, int nr_a, double scale_a_re, double scale_a_im, const void *e_b, size_t e_b_stride,
                      int ns_b, const void *x_b, size_t x_b_stride, int nr_b, double scale_b_re, double scale_b_im, int row_x,
                      int row_y, int row_z, const double *model_weights, size_t mw_stride, const double *volumes, double *out,
                      size_t ld, double *ws, size_t ws_len, void *stream)
{
    if (!e_a || !x_a || !e_b || !x_b || !model_weights || !volumes || !out || !ws)
        return fail(EMG3D_ERR_BADARG, "data_gram: null pointer");
    if (nx < 1 || ny < 1 || nz < 1 || ns_a < 1 || nr_a < 1 || ns_b < 1 || nr_b < 1)
        return fail(EMG3D_ERR_BADARG, "data_gram: a size is smaller than 1");
    if (row_x < 0 || row_x > 2 || row_y < 0 || row_y > 2 || row_z < 0 || row_z > 2)
        return fail(EMG3D_ERR_BADARG, "data_gram: a row index is outside 0..2");
    const size_t n_edges = (size_t)nx * (ny + 1) * (nz + 1) + (size_t)(nx + 1) * ny * (nz + 1) +
                           (size_t)(nx + 1) * (ny + 1) * nz;
    const size_t n_a = (size_t)ns_a * nr_a, n_b = (size_t)ns_b * nr_b, c = is_complex ? 2 : 1;
    if (e_a_stride < n_edges || x_a_stride < n_edges || e_b_stride < n_edges || x_b_stride < n_edges ||
        mw_stride < (size_t)nx * ny * nz || ld < c * n_b)
        return fail(EMG3D_ERR_BADARG, "data_gram: a stride is smaller than its row");
    const size_t tiles = (size_t)cdiv(ns_a, GR_TS) * cdiv(nr_a, GR_TR) * cdiv(ns_b, GR_TS) * cdiv(nr_b, GR_TR);
    if (n_a > 65535 * 8 || n_b > 65535 * 8 || tiles > 65535 || gram_patches(nx, ny, nz) > (size_t)INT_MAX)
        return fail(EMG3D_ERR_BADARG, "data_gram: too large for one launch (more than 65 535 pairs of tiles)");
    const size_t need = gram_ws_len(nx, ny, nz, is_complex, (int)n_a, (int)n_b);
    if (ws_len < need) return fail(EMG3D_ERR_BADARG, "data_gram: ws_len is below emg3d_data_gram_ws_len");
    // workgroups per pair of tiles: what the workspace of THESE sizes holds -- not what the caller passed
    const size_t R = (size_t)GR_DATA * c;
    const int n_wg = (int)std::min(std::min(gram_patches(nx, ny, nz), (size_t)GR_MAX_WG), need / (R * R * tiles));
    using SC = std::conditional_t<SP, emg::cplxf, cplx>;
    using SR = std::conditional_t<SP, float, double>;
    return is_complex ? data_gram<cplx, SC>(nx, ny, nz, e_a, e_a_stride, ns_a, x_a, x_a_stride, nr_a, scale_a_re, scale_a_im, e_b,
                                            e_b_stride, ns_b, x_b, x_b_stride, nr_b, scale_b_re, scale_b_im, n_wg, row_x, row_y,
                                            row_z, model_weights, mw_stride, volumes, out, ld, ws, (hipStream_t)stream)
                      : data_gram<double, SR>(nx, ny, nz, e_a, e_a_stride, ns_a, x_a, x_a_stride, nr_a, scale_a_re, scale_a_im,
                                              e_b, e_b_stride, ns_b, x_b, x_b_stride, nr_b, scale_b_re, scale_b_im, n_wg, row_x, row_y,
                                              row_z, model_weights, mw_stride, volumes, out, ld, ws, (hipStream_t)stream);
}

}  // namespace

extern "C" {

size_t emg3d_data_gram_ws_len(int nx, int ny, int nz, int is_complex, int n_a, int n_b)
{
    if (nx < 1 || ny < 1 || nz < 1 || n_a < 1 || n_b < 1) return 0;
    return gram_ws_len(nx, ny, nz, is_complex, n_a, n_b);
}

int emg3d_dev_data_gram(int nx, int ny, int nz, int is_complex, const void *e_a, size_t e_a_stride, int ns_a, const void *x_a,
                        size_t x_a_stride, int nr_a, double scale_a_re, double scale_a_im, const void *e_b, size_t e_b_stride,
                        int ns_b, const void *x_b, size_t x_b_stride, int nr_b, double scale_b_re, double scale_b_im, int row_x,
                        int row_y, int row_z, const double *model_weights, size_t mw_stride, const double *volumes, double *out,
                        size_t ld, double *ws, size_t ws_len, void *stream)
{
    return data_gram_checked<false>(nx, ny, nz, is_complex, e_a, e_a_stride, ns_a, x_a, x_a_stride, nr_a, scale_a_re,
                                    scale_a_im, e_b, e_b_stride, ns_b, x_b, x_b_stride, nr_b, scale_b_re, scale_b_im, row_x, row_y,
                                    row_z, model_weights, mw_stride, volumes, out, ld, ws, ws_len, stream);
}

int emg3d_dev_data_gram_sp(int nx, int ny, int nz, int is_complex, const void *e_a, size_t e_a_stride, int ns_a, const void *x_a,
                           size_t x_a_stride, int nr_a, double scale_a_re, double scale_a_im, const void *e_b, size_t e_b_stride,
                           int ns_b, const void *x_b, size_t x_b_stride, int nr_b, double scale_b_re, double scale_b_im, int row_x,
                           int row_y, int row_z, const double *model_weights, size_t mw_stride, const double *volumes, double *out,
                           size_t ld, double *ws, size_t ws_len, void *stream)
{
    return data_gram_checked<true>(nx, ny, nz, is_complex, e_a, e_a_stride, ns_a, x_a, x_a_stride, nr_a, scale_a_re,
                                   scale_a_im, e_b, e_b_stride, ns_b, x_b, x_b_stride, nr_b, scale_b_re, scale_b_im, row_x, row_y,
                                   row_z, model_weights, mw_stride, volumes, out, ld, ws, ws_len, stream);
}

}  // extern "C"
