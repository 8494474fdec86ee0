// The inner linear solve of a Gauss-Newton step, (Re J^H W J + lambda_k R) x_k = b_k for K dampings at once
// (DESIGN.md 4.17): the model regulariser R and the vector kernels of a block preconditioned CG whose K columns
// share every pass over the kept fields (block.h). Everything here is plain fp64 and bound by memory; there are no
// floating-point atomics, every sum runs in an order fixed by the sizes alone: the same call gives the same bits.
//
// R, the finite-volume smallness-plus-roughness operator on the model grid (cells x fastest), applied to every
// component of a vector independently:
//
//     (R v)[c] = a[c] ( alpha_s V_c v[c] + sum_{d = x,y,z} alpha_d sum_{faces f of c along d} a[c'] A_f / l_f (v[c] - v[c']) )
//
// V_c cell volume, A_f face area, l_f = (h_d[c] + h_d[c']) / 2 the distance of the two cell centres, a the 0 / 1 mask
// of the active cells; faces on the boundary of the grid or towards an inactive cell are left out, rows of inactive
// cells are 0. The coefficient of a face is formed from the widths by the same operations from either side (the sum
// of the two widths commutes): R is symmetric in floating point as stored, and v[c] - v[c'] = 0 for a constant.
//
//   k_model_regulariser       one thread per cell (x along the lanes, y / z neighbours through the cache). The seven
//                             coefficients of the cell are formed ONCE from the widths and the mask (never stored)
//                             and serve all nvec vectors, the vector loop innermost. A coefficient that is 0 (boundary,
//                             inactive neighbour) redirects its load to the cell itself: no branch, and nothing of an
//                             inactive cell is read as a neighbour. Per column (vec_per_col vectors) a wave adds its
//                             <p, q_new> with shuffles and writes ONE partial sum: ws[col * nwaves + wave], wave =
//                             4 * (linear workgroup index) + wave in the workgroup.
//   k_regulariser_finish      one workgroup per column: thread t adds the partials t, t + 256, ... in ascending order,
//                             then a binary tree over the 256 threads in LDS.
//   k_model_regulariser_diagonal   diag R from the same coefficients.
//   k_model_regulariser_weighted, k_model_regulariser_weighted_diagonal   the same two for the weighted / sparse-norm
//                             (IRLS) form of R (described where they stand): the coefficients carry
//                             cell weights and powers of the linearisation vector's values and gradients, per component.
//   k_pcg_update              grid (blocks, K). Column k, if its state is 0: alpha = <r,z> / <p,q>, x += alpha p,
//                             r -= alpha q (0 on inactive cells), z = M r with the Jacobi preconditioner M formed here
//                             from the two shared diagonals and the column's lambda, and the workgroup's share of
//                             <r, z> and <r, r> with the NEW r: ws[(k * blocks + block) * 2 + {0, 1}]. z is not stored
//                             (k_pcg_direction forms it again from r: 16 / K B per element for the diagonals instead of
//                             8 B written and 8 B read). A column whose state is not 0 is not touched at all.
//                             rdiag_stride: doubles between the diagonals of R of two components (0: one for all).
//   k_pcg_scalar              ONE workgroup: adds the partial sums (thread t takes t, t + 256, ..., then the LDS tree),
//                             advances the table and freezes a column whose state leaves 0.
//   k_pcg_direction           p = z + beta p, beta = <r,z> / <r,z>_old (first: p = z), columns of state 0 only.
//
// The table: PCG_ROW = 8 doubles per column,
//     [0] lambda  [1] <b,b>  [2] <r,z>  [3] <r,z> of the iteration before  [4] <p,q>  [5] <r,r>  [6] iterations  [7] state
// state 0 running, 1 converged (<r,r> <= tol^2 <b,b>), 2 breakdown (<p,q> <= 0, or <r,z> <= 0 with r != 0), 3 a sum is
// not finite. Frozen columns (state != 0) are skipped by k_pcg_update and k_pcg_direction: x, r and p keep their bits
// however long the other columns iterate.
// Included at the end of kernels.hip (one translation unit).
#pragma once

namespace {

constexpr int PCG_ROW = 8, PCG_BLOCK = 256, PCG_GRID = 1024;
enum { PCG_LAM = 0, PCG_BB = 1, PCG_RZ = 2, PCG_RZ_OLD = 3, PCG_PQ = 4, PCG_RR = 5, PCG_IT = 6, PCG_STATE = 7 };

struct RegGeo {
    int nx, ny, nz;
    const double *hx, *hy, *hz;
    double as, ax, ay, az;
    const unsigned char *mask;
};

// The coefficients of cell (ix, iy, iz), c = ix + nx (iy + ny iz): cs = alpha_s V_c, cf[f] = alpha_d a[c'] A_f / l_f for
// the faces f = x-, x+, y-, y+, z-, z+ and off[f] = c' - c (0 where cf[f] = 0). Returns a[c].
__device__ __forceinline__ bool reg_coefs(const RegGeo &G, int ix, int iy, int iz, size_t c, double &cs, double (&cf)[6],
                                          int (&off)[6])
{
    const double hx = G.hx[ix], hy = G.hy[iy], hz = G.hz[iz];
    const int sy = G.nx, sz = G.nx * G.ny;
    const unsigned char *m = G.mask;
    cs = G.as * (hx * hy * hz);
    const double fx = G.ax * (hy * hz), fy = G.ay * (hx * hz), fz = G.az * (hx * hy);
    const bool has[6] = {ix > 0 && (!m || m[c - 1]),      ix + 1 < G.nx && (!m || m[c + 1]),
                         iy > 0 && (!m || m[c - sy]),     iy + 1 < G.ny && (!m || m[c + sy]),
                         iz > 0 && (!m || m[c - sz]),     iz + 1 < G.nz && (!m || m[c + sz])};
    cf[0] = has[0] ? fx / (0.5 * (G.hx[has[0] ? ix - 1 : ix] + hx)) : 0.0;
    cf[1] = has[1] ? fx / (0.5 * (G.hx[has[1] ? ix + 1 : ix] + hx)) : 0.0;
    cf[2] = has[2] ? fy / (0.5 * (G.hy[has[2] ? iy - 1 : iy] + hy)) : 0.0;
    cf[3] = has[3] ? fy / (0.5 * (G.hy[has[3] ? iy + 1 : iy] + hy)) : 0.0;
    cf[4] = has[4] ? fz / (0.5 * (G.hz[has[4] ? iz - 1 : iz] + hz)) : 0.0;
    cf[5] = has[5] ? fz / (0.5 * (G.hz[has[5] ? iz + 1 : iz] + hz)) : 0.0;
    off[0] = has[0] ? -1 : 0;   off[1] = has[1] ? 1 : 0;
    off[2] = has[2] ? -sy : 0;  off[3] = has[3] ? sy : 0;
    off[4] = has[4] ? -sz : 0;  off[5] = has[5] ? sz : 0;
    return !m || m[c];
}

__device__ __forceinline__ double wave_sum(double a)
{
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
    return a;
}

__global__ __launch_bounds__(256) void k_model_regulariser(RegGeo G, int ncol, int vpc, const double *__restrict__ p,
                                                           double *__restrict__ q, double beta,
                                                           const double *__restrict__ lam, double *ws)
{
    const int ix = blockIdx.x * 64 + threadIdx.x, iy = blockIdx.y * 4 + threadIdx.y, iz = blockIdx.z;
    const bool inside = ix < G.nx && iy < G.ny;
    const size_t ncell = (size_t)G.nx * G.ny * G.nz;
    const size_t c = inside ? (size_t)ix + (size_t)G.nx * ((size_t)iy + (size_t)G.ny * iz) : 0;
    double cs = 0.0, cf[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int off[6] = {0, 0, 0, 0, 0, 0};
    bool act = false;
    if (inside) act = reg_coefs(G, ix, iy, iz, c, cs, cf, off);
    const size_t nwaves = (size_t)gridDim.x * gridDim.y * gridDim.z * 4;
    const size_t wave = ((size_t)blockIdx.x + (size_t)gridDim.x * ((size_t)blockIdx.y + (size_t)gridDim.y * blockIdx.z)) * 4 +
                        threadIdx.y;
    for (int col = 0; col < ncol; ++col) {
        const double l = lam ? lam[col] : 1.0;
        double acc = 0.0;
        if (inside) {
            for (int k = 0; k < vpc; ++k) {
                const size_t base = ((size_t)col * vpc + k) * ncell + c;
                const double *pc = p + base;
                const double v = pc[0];
                double r = cs * v;
#pragma unroll
                for (int f = 0; f < 6; ++f) r += cf[f] * (v - pc[off[f]]);
                r = act ? r : 0.0;
                const double qn = beta != 0.0 ? beta * q[base] + l * r : l * r;
                q[base] = qn;
                acc += v * qn;
            }
        }
        if (ws) {
            acc = wave_sum(acc);
            if (threadIdx.x == 0) ws[(size_t)col * nwaves + wave] = acc;
        }
    }
}

// out[col] = sum of the nparts partials of column col (one workgroup per column)
__global__ __launch_bounds__(PCG_BLOCK) void k_regulariser_finish(const double *__restrict__ ws, size_t nparts, double *out)
{
    __shared__ double sm[PCG_BLOCK];
    const double *w = ws + (size_t)blockIdx.x * nparts;
    double a = 0.0;
    for (size_t i = threadIdx.x; i < nparts; i += PCG_BLOCK) a += w[i];
    sm[threadIdx.x] = a;
    __syncthreads();
    for (int s = PCG_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sm[0];
}

__global__ __launch_bounds__(256) void k_model_regulariser_diagonal(RegGeo G, double *diag)
{
    const int ix = blockIdx.x * 64 + threadIdx.x, iy = blockIdx.y * 4 + threadIdx.y, iz = blockIdx.z;
    if (ix >= G.nx || iy >= G.ny) return;
    const size_t c = (size_t)ix + (size_t)G.nx * ((size_t)iy + (size_t)G.ny * iz);
    double cs, cf[6];
    int off[6];
    const bool act = reg_coefs(G, ix, iy, iz, c, cs, cf, off);
    double d = cs;
#pragma unroll
    for (int f = 0; f < 6; ++f) d += cf[f];
    diag[c] = act ? d : 0.0;
}

// ---- the weighted / sparse-norm (IRLS) operator ----
// Component k of a column has cell weights w_k >= 0 and linearisation values u_k, both shared by all columns:
//
//     cs[c]   = alpha_s V_c        w[c]               rho(p_s, eps_s; u[c])
//     cf[c,f] = (coefficient of reg_coefs) (w[c] + w[c']) / 2  rho(p_d, eps_g; (u[c] - u[c']) / l_f)
//     rho(p, eps; t) = (t^2 + eps^2)^(p / 2 - 1), and 1 -- nothing read, nothing multiplied -- for p = 2.
//
// Every factor of a face comes out the same from either side (w[c] + w[c'] commutes, t enters as fma(t, t, eps^2) and
// (-t)(-t) = t t), and the factors are multiplied in one order: R stays symmetric as stored and >= 0.
struct RegW {
    const double *w, *u;        // NULL: weights 1; no linearisation (all norms 2)
    size_t wstride, ustride;    // doubles between the components' rows; 0: one row for all
    double ps, px, py, pz;      // the norms of the smallness term and of the three directions
    double es2, eg2;            // eps_s^2, eps_g^2
};

// rho(p, .; t) for p != 2, x2 = t^2 + eps^2 > 0: p = 1 and p = 0 without the power function
__device__ __forceinline__ double reg_rho(double p, double x2)
{
    if (p == 1.0) return 1.0 / sqrt(x2);
    if (p == 0.0) return 1.0 / x2;
    return pow(x2, 0.5 * p - 1.0);
}

// reg_coefs for component k with the weights and the norms worked in. A face whose coefficient is 0 has off[f] = 0:
// its w and u are those of the cell itself, nothing of an inactive cell or past the grid is read.
// es = w[c] rho(p_s, eps_s; u[c]), the factor that cs carries on top of alpha_s V_c (exactly 1 without weights and with
// p_s = 2).
__device__ __forceinline__ bool reg_coefs_weighted(const RegGeo &G, const RegW &W, int k, int ix, int iy, int iz, size_t c,
                                                   double &cs, double &es, double (&cf)[6], int (&off)[6])
{
    const bool act = reg_coefs(G, ix, iy, iz, c, cs, cf, off);
    const double *w = W.w ? W.w + (size_t)k * W.wstride + c : nullptr;
    const double *u = W.u ? W.u + (size_t)k * W.ustride + c : nullptr;
    es = 1.0;
    if (w) {
        const double wc = w[0];
        es = wc;
#pragma unroll
        for (int f = 0; f < 6; ++f) cf[f] *= 0.5 * (wc + w[off[f]]);
    }
    if (W.ps != 2.0) es *= reg_rho(W.ps, fma(u[0], u[0], W.es2));
    cs *= es;
    const double pd[3] = {W.px, W.py, W.pz};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (pd[d] == 2.0) continue;
        const double hc = d == 0 ? G.hx[ix] : d == 1 ? G.hy[iy] : G.hz[iz];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int f = 2 * d + s;
            const int j = (d == 0 ? ix : d == 1 ? iy : iz) + (off[f] == 0 ? 0 : s ? 1 : -1);
            const double hn = d == 0 ? G.hx[j] : d == 1 ? G.hy[j] : G.hz[j];
            const double t = (u[0] - u[off[f]]) / (0.5 * (hn + hc));
            cf[f] *= reg_rho(pd[d], fma(t, t, W.eg2));
        }
    }
    return act;
}

// k_model_regulariser with the coefficients of all VPC components formed up front in registers (VPC x 7 doubles), then
// the same column-outer / component-inner loop: the same seven additions in the same order, the same partial sums.
// With weights of 1 and norms of 2 the bits must be those of k_model_regulariser, and which products the compiler fuses
// into which sums differs from kernel to kernel (here: beta q + l r came out as fma(beta, q, l r), there as fma(l, r,
// beta q)). So contraction is off in this kernel and the loop spells out the operations that k_model_regulariser
// compiles to: cf[0] (v - p0), then cs v fused onto it, then the faces 1 .. 5 fused on one after the other; beta q,
// then l r fused onto it; v q_new fused onto the wave's sum. test_weighted_regulariser.py holds the two to each other.
template <int VPC>
__global__ __launch_bounds__(256) void k_model_regulariser_weighted(RegGeo G, RegW W, int ncol, const double *__restrict__ p,
                                                                    double *__restrict__ q, double beta,
                                                                    const double *__restrict__ lam, double *ws)
{
#pragma clang fp contract(off)
    const int ix = blockIdx.x * 64 + threadIdx.x, iy = blockIdx.y * 4 + threadIdx.y, iz = blockIdx.z;
    const bool inside = ix < G.nx && iy < G.ny;
    const size_t ncell = (size_t)G.nx * G.ny * G.nz;
    const size_t c = inside ? (size_t)ix + (size_t)G.nx * ((size_t)iy + (size_t)G.ny * iz) : 0;
    double cs[VPC], cf[VPC][6];
    int off[6] = {0, 0, 0, 0, 0, 0};
    bool act = false;
#pragma unroll
    for (int k = 0; k < VPC; ++k) {
        cs[k] = 0.0;
#pragma unroll
        for (int f = 0; f < 6; ++f) cf[k][f] = 0.0;
        double es;
        if (inside) act = reg_coefs_weighted(G, W, k, ix, iy, iz, c, cs[k], es, cf[k], off);
    }
    const size_t nwaves = (size_t)gridDim.x * gridDim.y * gridDim.z * 4;
    const size_t wave = ((size_t)blockIdx.x + (size_t)gridDim.x * ((size_t)blockIdx.y + (size_t)gridDim.y * blockIdx.z)) * 4 +
                        threadIdx.y;
    for (int col = 0; col < ncol; ++col) {
        const double l = lam ? lam[col] : 1.0;
        double acc = 0.0;
        if (inside) {
#pragma unroll
            for (int k = 0; k < VPC; ++k) {
                const size_t base = ((size_t)col * VPC + k) * ncell + c;
                const double *pc = p + base;
                const double v = pc[0];
                double r = fma(cs[k], v, cf[k][0] * (v - pc[off[0]]));
#pragma unroll
                for (int f = 1; f < 6; ++f) r = fma(cf[k][f], v - pc[off[f]], r);
                r = act ? r : 0.0;
                const double qn = beta != 0.0 ? fma(l, r, beta * q[base]) : l * r;
                q[base] = qn;
                acc = fma(v, qn, acc);
            }
        }
        if (ws) {
            acc = wave_sum(acc);
            if (threadIdx.x == 0) ws[(size_t)col * nwaves + wave] = acc;
        }
    }
}

// diag[k * ncell + c] = (R_k)_cc, k < vpc. As above, spelled out: k_model_regulariser_diagonal compiles its first sum
// to fma(alpha_s, V_c, cf[0]), so here it is fma(alpha_s, V_c es, cf[0]) -- the same bits when es is exactly 1.
__global__ __launch_bounds__(256) void k_model_regulariser_weighted_diagonal(RegGeo G, RegW W, int vpc, double *diag)
{
#pragma clang fp contract(off)
    const int ix = blockIdx.x * 64 + threadIdx.x, iy = blockIdx.y * 4 + threadIdx.y, iz = blockIdx.z;
    if (ix >= G.nx || iy >= G.ny) return;
    const size_t ncell = (size_t)G.nx * G.ny * G.nz;
    const size_t c = (size_t)ix + (size_t)G.nx * ((size_t)iy + (size_t)G.ny * iz);
    for (int k = 0; k < vpc; ++k) {
        double cs, es, cf[6];
        int off[6];
        const bool act = reg_coefs_weighted(G, W, k, ix, iy, iz, c, cs, es, cf, off);
        double d = fma(G.as, G.hx[ix] * G.hy[iy] * G.hz[iz] * es, cf[0]);
#pragma unroll
        for (int f = 1; f < 6; ++f) d += cf[f];
        diag[(size_t)k * ncell + c] = act ? d : 0.0;
    }
}

// z = M r for one element: Jacobi 1 / (hdiag + lambda rdiag) (hdiag: of the element, rdiag: of its cell), the identity
// without diagonals or where the sum is not positive; 0 on inactive cells
__device__ __forceinline__ double pcg_precondition(double r, bool act, bool jacobi, double hd, double rd, double lam)
{
    if (!act) return 0.0;
    if (!jacobi) return r;
    const double d = hd + lam * rd;
    return d > 0.0 ? r / d : r;
}

__device__ __forceinline__ bool pcg_pq_ok(double pq) { return pq > 0.0 && pq <= 1.7976931348623157e308; }

__global__ __launch_bounds__(PCG_BLOCK) void k_pcg_update(size_t ncell, int vpc, int first, double *x, double *r,
                                                          const double *__restrict__ p, const double *__restrict__ q,
                                                          const double *__restrict__ hdiag, const double *__restrict__ rdiag,
                                                          size_t rdiag_stride, const unsigned char *__restrict__ mask,
                                                          const double *table, const double *pq, double *ws)
{
    const int col = blockIdx.y;
    const double *row = table + (size_t)col * PCG_ROW;
    const double lam = row[PCG_LAM];
    const bool run = row[PCG_STATE] == 0.0 && (first || pcg_pq_ok(pq[col]));
    const double alpha = (run && !first) ? row[PCG_RZ] / pq[col] : 0.0;
    double arz = 0.0, arr = 0.0;
    if (run) {
        for (int k = 0; k < vpc; ++k) {
            const size_t comp = (size_t)k * ncell, rcomp = (size_t)k * rdiag_stride, base = ((size_t)col * vpc + k) * ncell;
            for (size_t c = (size_t)blockIdx.x * PCG_BLOCK + threadIdx.x; c < ncell; c += (size_t)gridDim.x * PCG_BLOCK) {
                const bool act = !mask || mask[c];
                double rn = r[base + c];
                if (!first) {
                    x[base + c] += alpha * p[base + c];
                    rn -= alpha * q[base + c];
                }
                rn = act ? rn : 0.0;
                r[base + c] = rn;
                const double z = pcg_precondition(rn, act, hdiag != nullptr, hdiag ? hdiag[comp + c] : 0.0,
                                                  hdiag ? rdiag[rcomp + c] : 0.0, lam);
                arz += rn * z;
                arr += rn * rn;
            }
        }
    }
    __shared__ double sm[PCG_BLOCK / 64][2];
    arz = wave_sum(arz);
    arr = wave_sum(arr);
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = arz; sm[threadIdx.x >> 6][1] = arr; }
    __syncthreads();
    if (threadIdx.x < 2)
        ws[((size_t)col * gridDim.x + blockIdx.x) * 2 + threadIdx.x] =
            (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
}

__global__ __launch_bounds__(PCG_BLOCK) void k_pcg_scalar(int ncol, int nblocks, int first, double tol2, double *table,
                                                          const double *pq, const double *__restrict__ ws)
{
    __shared__ double sm[PCG_BLOCK];
    for (int col = 0; col < ncol; ++col) {
        double *row = table + (size_t)col * PCG_ROW;
        double sums[2];
        for (int part = 0; part < 2; ++part) {
            double a = 0.0;
            for (int b = threadIdx.x; b < nblocks; b += PCG_BLOCK) a += ws[((size_t)col * nblocks + b) * 2 + part];
            sm[threadIdx.x] = a;
            __syncthreads();
            for (int s = PCG_BLOCK / 2; s > 0; s >>= 1) {
                if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
                __syncthreads();
            }
            sums[part] = sm[0];
            __syncthreads();
        }
        if (threadIdx.x != 0 || row[PCG_STATE] != 0.0) continue;
        const double rz = sums[0], rr = sums[1];
        const bool finite = fabs(rz) <= 1.7976931348623157e308 && fabs(rr) <= 1.7976931348623157e308;
        if (first) {
            row[PCG_BB] = rr; row[PCG_RZ] = rz; row[PCG_RZ_OLD] = 0.0; row[PCG_PQ] = 0.0; row[PCG_RR] = rr; row[PCG_IT] = 0.0;
            row[PCG_STATE] = !finite ? 3.0 : rr == 0.0 ? 1.0 : !(rz > 0.0) ? 2.0 : 0.0;
            continue;
        }
        const double d = pq[col];
        row[PCG_PQ] = d;
        if (!pcg_pq_ok(d)) {                     // k_pcg_update has left the column as it was
            row[PCG_STATE] = d <= 0.0 ? 2.0 : 3.0;
            continue;
        }
        row[PCG_RZ_OLD] = row[PCG_RZ];
        row[PCG_RZ] = rz;
        row[PCG_RR] = rr;
        row[PCG_IT] += 1.0;
        row[PCG_STATE] = !finite ? 3.0 : rr <= tol2 * row[PCG_BB] ? 1.0 : !(rz > 0.0) ? 2.0 : 0.0;
    }
}

__global__ __launch_bounds__(PCG_BLOCK) void k_pcg_direction(size_t ncell, int vpc, int first, double *p,
                                                             const double *__restrict__ r, const double *__restrict__ hdiag,
                                                             const double *__restrict__ rdiag, size_t rdiag_stride,
                                                             const unsigned char *__restrict__ mask, const double *table)
{
    const int col = blockIdx.y;
    const double *row = table + (size_t)col * PCG_ROW;
    if (row[PCG_STATE] != 0.0) return;
    const double lam = row[PCG_LAM];
    const double beta = first ? 0.0 : row[PCG_RZ] / row[PCG_RZ_OLD];
    for (int k = 0; k < vpc; ++k) {
        const size_t comp = (size_t)k * ncell, rcomp = (size_t)k * rdiag_stride, base = ((size_t)col * vpc + k) * ncell;
        for (size_t c = (size_t)blockIdx.x * PCG_BLOCK + threadIdx.x; c < ncell; c += (size_t)gridDim.x * PCG_BLOCK) {
            const bool act = !mask || mask[c];
            const double z = pcg_precondition(r[base + c], act, hdiag != nullptr, hdiag ? hdiag[comp + c] : 0.0,
                                              hdiag ? rdiag[rcomp + c] : 0.0, lam);
            p[base + c] = first ? z : z + beta * p[base + c];
        }
    }
}

inline int pcg_blocks(size_t ncell)
{
    const size_t want = (ncell + PCG_BLOCK - 1) / PCG_BLOCK;
    return (int)(want < 1 ? 1 : want > (size_t)PCG_GRID ? (size_t)PCG_GRID : want);
}
inline bool reg_sizes_ok(int nx, int ny, int nz)
{
    return nx >= 1 && ny >= 1 && nz >= 1 && (long long)nx * ny * nz < (1LL << 31) && nz <= 65535 && (ny + 3) / 4 <= 65535;
}
inline size_t reg_waves(int nx, int ny, int nz) { return (size_t)((nx + 63) / 64) * ((ny + 3) / 4) * nz * 4; }

// The weights, the linearisation and the norms of the weighted entries: 0 and W filled, or the error
inline int reg_weighted_args(const char *who, size_t ncell, const double *cell_weights, size_t weights_stride,
                             const double *linearise_at, size_t linearise_stride, double p_s, double p_x, double p_y, double p_z,
                             double eps_s, double eps_g, RegW &W)
{
    const double ps[4] = {p_s, p_x, p_y, p_z};
    bool sparse = false;
    for (double e : ps) {
        if (!(e >= 0.0 && e <= 2.0)) return fail(EMG3D_ERR_BADARG, (std::string(who) + ": a norm is not in [0, 2]").c_str());
        sparse = sparse || e != 2.0;
    }
    if (sparse && !linearise_at)
        return fail(EMG3D_ERR_BADARG, (std::string(who) + ": a norm other than 2 needs linearise_at").c_str());
    if (sparse && !(eps_s > 0.0 && eps_s <= 1.7976931348623157e308 && eps_g > 0.0 && eps_g <= 1.7976931348623157e308))
        return fail(EMG3D_ERR_BADARG, (std::string(who) + ": a norm other than 2 needs finite thresholds eps_s, eps_g > 0").c_str());
    if ((weights_stride != 0 && weights_stride < ncell) || (linearise_stride != 0 && linearise_stride < ncell))
        return fail(EMG3D_ERR_BADARG, (std::string(who) + ": a stride is neither 0 nor >= nx ny nz").c_str());
    W = {cell_weights, sparse ? linearise_at : nullptr, weights_stride, linearise_stride, p_s, p_x, p_y, p_z,
         sparse ? eps_s * eps_s : 0.0, sparse ? eps_g * eps_g : 0.0};
    return 0;
}

}  // namespace

extern "C" {

size_t emg3d_model_regulariser_ws_len(int nx, int ny, int nz, int nvec, int vec_per_col)
{
    if (!reg_sizes_ok(nx, ny, nz) || nvec < 1 || vec_per_col < 1 || nvec % vec_per_col != 0) return 0;
    return (size_t)(nvec / vec_per_col) * reg_waves(nx, ny, nz);
}

int emg3d_dev_model_regulariser(int nx, int ny, int nz, const double *hx, const double *hy, const double *hz,
                                double alpha_s, double alpha_x, double alpha_y, double alpha_z, const unsigned char *mask,
                                int nvec, int vec_per_col, const double *p, double *q, double beta, const double *lam,
                                double *pq, double *ws, size_t ws_len, void *stream)
{
    if (!reg_sizes_ok(nx, ny, nz) || !hx || !hy || !hz || nvec < 1 || vec_per_col < 1 || nvec % vec_per_col != 0 || !p || !q ||
        p == q || nvec / vec_per_col > 65535)
        return fail(EMG3D_ERR_BADARG, "model_regulariser: bad argument");
    if (pq && (!ws || ws_len < emg3d_model_regulariser_ws_len(nx, ny, nz, nvec, vec_per_col)))
        return fail(EMG3D_ERR_SCRATCH, "model_regulariser: workspace too small (emg3d_model_regulariser_ws_len)");
    const RegGeo G = {nx, ny, nz, hx, hy, hz, alpha_s, alpha_x, alpha_y, alpha_z, mask};
    const int ncol = nvec / vec_per_col;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_model_regulariser, dim3((nx + 63) / 64, (ny + 3) / 4, nz), dim3(64, 4, 1), 0, st, G, ncol, vec_per_col,
                       p, q, beta, lam, pq ? ws : (double *)nullptr);
    if (pq)
        hipLaunchKernelGGL(k_regulariser_finish, dim3(ncol), dim3(PCG_BLOCK), 0, st, (const double *)ws, reg_waves(nx, ny, nz),
                           pq);
    HIP_TRY(hipGetLastError());
    return 0;
}

int emg3d_dev_model_regulariser_diagonal(int nx, int ny, int nz, const double *hx, const double *hy, const double *hz,
                                         double alpha_s, double alpha_x, double alpha_y, double alpha_z,
                                         const unsigned char *mask, double *diag, void *stream)
{
    if (!reg_sizes_ok(nx, ny, nz) || !hx || !hy || !hz || !diag)
        return fail(EMG3D_ERR_BADARG, "model_regulariser_diagonal: bad argument");
    const RegGeo G = {nx, ny, nz, hx, hy, hz, alpha_s, alpha_x, alpha_y, alpha_z, mask};
    hipLaunchKernelGGL(k_model_regulariser_diagonal, dim3((nx + 63) / 64, (ny + 3) / 4, nz), dim3(64, 4, 1), 0,
                       (hipStream_t)stream, G, diag);
    HIP_TRY(hipGetLastError());
    return 0;
}

int emg3d_dev_model_regulariser_weighted(int nx, int ny, int nz, const double *hx, const double *hy, const double *hz,
                                         double alpha_s, double alpha_x, double alpha_y, double alpha_z,
                                         const unsigned char *mask, const double *cell_weights, size_t weights_stride,
                                         const double *linearise_at, size_t linearise_stride, double p_s, double p_x,
                                         double p_y, double p_z, double eps_s, double eps_g, int nvec, int vec_per_col,
                                         const double *p, double *q, double beta, const double *lam, double *pq, double *ws,
                                         size_t ws_len, void *stream)
{
    if (!reg_sizes_ok(nx, ny, nz) || !hx || !hy || !hz || nvec < 1 || vec_per_col < 1 || vec_per_col > 3 ||
        nvec % vec_per_col != 0 || !p || !q || p == q || nvec / vec_per_col > 65535)
        return fail(EMG3D_ERR_BADARG, "model_regulariser_weighted: bad argument");
    RegW W;
    if (int err = reg_weighted_args("model_regulariser_weighted", (size_t)nx * ny * nz, cell_weights, weights_stride,
                                    linearise_at, linearise_stride, p_s, p_x, p_y, p_z, eps_s, eps_g, W))
        return err;
    if (pq && (!ws || ws_len < emg3d_model_regulariser_ws_len(nx, ny, nz, nvec, vec_per_col)))
        return fail(EMG3D_ERR_SCRATCH, "model_regulariser_weighted: workspace too small (emg3d_model_regulariser_ws_len)");
    const RegGeo G = {nx, ny, nz, hx, hy, hz, alpha_s, alpha_x, alpha_y, alpha_z, mask};
    const int ncol = nvec / vec_per_col;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((nx + 63) / 64, (ny + 3) / 4, nz), block(64, 4, 1);
    double *wsp = pq ? ws : (double *)nullptr;
    if (vec_per_col == 1)
        hipLaunchKernelGGL(k_model_regulariser_weighted<1>, grid, block, 0, st, G, W, ncol, p, q, beta, lam, wsp);
    else if (vec_per_col == 2)
        hipLaunchKernelGGL(k_model_regulariser_weighted<2>, grid, block, 0, st, G, W, ncol, p, q, beta, lam, wsp);
    else
        hipLaunchKernelGGL(k_model_regulariser_weighted<3>, grid, block, 0, st, G, W, ncol, p, q, beta, lam, wsp);
    if (pq)
        hipLaunchKernelGGL(k_regulariser_finish, dim3(ncol), dim3(PCG_BLOCK), 0, st, (const double *)ws, reg_waves(nx, ny, nz),
                           pq);
    HIP_TRY(hipGetLastError());
    return 0;
}

int emg3d_dev_model_regulariser_weighted_diagonal(int nx, int ny, int nz, const double *hx, const double *hy,
                                                  const double *hz, double alpha_s, double alpha_x, double alpha_y,
                                                  double alpha_z, const unsigned char *mask, const double *cell_weights,
                                                  size_t weights_stride, const double *linearise_at, size_t linearise_stride,
                                                  double p_s, double p_x, double p_y, double p_z, double eps_s, double eps_g,
                                                  int vec_per_col, double *diag, void *stream)
{
    if (!reg_sizes_ok(nx, ny, nz) || !hx || !hy || !hz || !diag || vec_per_col < 1 || vec_per_col > 3)
        return fail(EMG3D_ERR_BADARG, "model_regulariser_weighted_diagonal: bad argument");
    RegW W;
    if (int err = reg_weighted_args("model_regulariser_weighted_diagonal", (size_t)nx * ny * nz, cell_weights, weights_stride,
                                    linearise_at, linearise_stride, p_s, p_x, p_y, p_z, eps_s, eps_g, W))
        return err;
    const RegGeo G = {nx, ny, nz, hx, hy, hz, alpha_s, alpha_x, alpha_y, alpha_z, mask};
    hipLaunchKernelGGL(k_model_regulariser_weighted_diagonal, dim3((nx + 63) / 64, (ny + 3) / 4, nz), dim3(64, 4, 1), 0,
                       (hipStream_t)stream, G, W, vec_per_col, diag);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t emg3d_pcg_table_len(int ncol) { return ncol < 1 ? 0 : (size_t)ncol * PCG_ROW; }

size_t emg3d_pcg_ws_len(size_t n_cells, int ncol)
{
    if (n_cells < 1 || ncol < 1) return 0;
    return (size_t)ncol * pcg_blocks(n_cells) * 2;
}

int emg3d_dev_pcg_update_rd(size_t n_cells, int vec_per_col, int ncol, int first, double *x, double *r, const double *p,
                            const double *q, const double *hdiag, const double *rdiag, size_t rdiag_stride,
                            const unsigned char *mask, const double *table, const double *pq, double *ws, size_t ws_len,
                            void *stream)
{
    if (n_cells < 1 || vec_per_col < 1 || ncol < 1 || ncol > 65535 || !r || !table || !ws || (hdiag && !rdiag) ||
        (rdiag_stride != 0 && rdiag_stride < n_cells) || (!first && (!x || !p || !q || !pq)))
        return fail(EMG3D_ERR_BADARG, "pcg_update: bad argument");
    if (ws_len < emg3d_pcg_ws_len(n_cells, ncol))
        return fail(EMG3D_ERR_SCRATCH, "pcg_update: workspace too small (emg3d_pcg_ws_len)");
    hipLaunchKernelGGL(k_pcg_update, dim3(pcg_blocks(n_cells), ncol), dim3(PCG_BLOCK), 0, (hipStream_t)stream, n_cells,
                       vec_per_col, first ? 1 : 0, x, r, p, q, hdiag, rdiag, rdiag_stride, mask, table, pq, ws);
    HIP_TRY(hipGetLastError());
    return 0;
}

int emg3d_dev_pcg_update(size_t n_cells, int vec_per_col, int ncol, int first, double *x, double *r, const double *p,
                         const double *q, const double *hdiag, const double *rdiag, const unsigned char *mask,
                         const double *table, const double *pq, double *ws, size_t ws_len, void *stream)
{
    return emg3d_dev_pcg_update_rd(n_cells, vec_per_col, ncol, first, x, r, p, q, hdiag, rdiag, 0, mask, table, pq, ws, ws_len,
                                   stream);
}

int emg3d_dev_pcg_scalar(size_t n_cells, int ncol, int first, double tol, double *table, const double *pq, const double *ws,
                         size_t ws_len, void *stream)
{
    if (n_cells < 1 || ncol < 1 || !table || !ws || (!first && !pq) || !(tol >= 0.0))
        return fail(EMG3D_ERR_BADARG, "pcg_scalar: bad argument");
    if (ws_len < emg3d_pcg_ws_len(n_cells, ncol))
        return fail(EMG3D_ERR_SCRATCH, "pcg_scalar: workspace too small (emg3d_pcg_ws_len)");
    hipLaunchKernelGGL(k_pcg_scalar, dim3(1), dim3(PCG_BLOCK), 0, (hipStream_t)stream, ncol, pcg_blocks(n_cells), first ? 1 : 0,
                       tol * tol, table, pq, ws);
    HIP_TRY(hipGetLastError());
    return 0;
}

int emg3d_dev_pcg_direction_rd(size_t n_cells, int vec_per_col, int ncol, int first, double *p, const double *r,
                               const double *hdiag, const double *rdiag, size_t rdiag_stride, const unsigned char *mask,
                               const double *table, void *stream)
{
    if (n_cells < 1 || vec_per_col < 1 || ncol < 1 || ncol > 65535 || !p || !r || !table || (hdiag && !rdiag) ||
        (rdiag_stride != 0 && rdiag_stride < n_cells))
        return fail(EMG3D_ERR_BADARG, "pcg_direction: bad argument");
    hipLaunchKernelGGL(k_pcg_direction, dim3(pcg_blocks(n_cells), ncol), dim3(PCG_BLOCK), 0, (hipStream_t)stream, n_cells,
                       vec_per_col, first ? 1 : 0, p, r, hdiag, rdiag, rdiag_stride, mask, table);
    HIP_TRY(hipGetLastError());
    return 0;
}

int emg3d_dev_pcg_direction(size_t n_cells, int vec_per_col, int ncol, int first, double *p, const double *r,
                            const double *hdiag, const double *rdiag, const unsigned char *mask, const double *table,
                            void *stream)
{
    return emg3d_dev_pcg_direction_rd(n_cells, vec_per_col, ncol, first, p, r, hdiag, rdiag, 0, mask, table, stream);
}

}  // extern "C"
