// Block sensitivity products: the two reductions of reciprocal.h for nv vectors per pass over the
// kept stacks,
//     dots_block:    out[v, s, r] = scale sum_k w_v[k] e_s[k] x_r[k]             w: nv real rows, w_stride apart
//     combine_block: t_v[k]       = sum_s e_s[k] (sum_r coef[v, s, r] x_r[k])    t: nv rows, t_stride apart
// The stacks are the same for every vector: a workgroup loads a field value once and uses it for every vector of its
// tile. Plain fp64, no atomics, every sum in an order fixed by the sizes (and, for narrow stacks, by the one bit
// "16-byte loads"); nothing behind n is read in any row, nothing between the rows of t is written.
// Included at the end of kernels.hip, after reciprocal.h, whose chunks, packs, final sum and alignment rule it shares.
#pragma once

namespace {

// ---- dots_block. Per k the products p[i][j] = e_i[k] x_j[k] of a DB_TS x DB_TR tile are formed ONCE and added into
// the accumulators of DB_TV vectors, acc[v][i][j] += w_v[k] p[i][j]: 4 + 2 DB_TV fused operations per complex pair and
// k instead of the 6 of k_sensitivity_dots per vector. The tile is bounded by registers: DB_TV * DB_TS * DB_TR = 32
// complex accumulators are 128 VGPRs, what leaves room for the loads of two k in flight below 256 -- two waves per
// SIMD, a workgroup of 8 per compute unit; 4 x 4 x 4 would need 256 for the accumulators alone. A tile belongs to ONE WAVE, which streams a whole chunk
// for it, and the (up to DB_WAVES) waves of a workgroup take different tiles of the SAME chunk: they ask for the same
// field values at about the same time on the same compute unit, so a value comes from HBM once and from the caches of
// that unit for the other tiles. No LDS, no barrier: a wave reduces by shuffles and lane 0 writes its partials. Stage 2
// is k_sensitivity_dots_final with one workgroup per (v, s, r).
constexpr int DB_TS = 2, DB_TR = 4, DB_TV = 4, DB_WAVES = 8, DB_UNROLL = 2;
constexpr size_t DB_CHUNK = 4096;           // elements of k per wave: 64 per lane; half of DOT_CHUNK, as a workgroup of up
                                            // to 8 waves fills a compute unit and a launch should be many rounds of them

template <class T>
__device__ __forceinline__ void dots_block_fma(const double (&wk)[DB_TV], const T (&ev)[DB_TS], const T (&xv)[DB_TR],
                                               T (&acc)[DB_TV][DB_TS][DB_TR])
{
#pragma unroll
    for (int i = 0; i < DB_TS; ++i)
#pragma unroll
        for (int j = 0; j < DB_TR; ++j) {
            const T p = ev[i] * xv[j];
#pragma unroll
            for (int v = 0; v < DB_TV; ++v) acc[v][i][j] = emg::mad(wk[v], p, acc[v][i][j]);
        }
}

// One k of the tile, element-wise loads.
template <class T, class S>
__device__ __forceinline__ void dots_block_step(size_t k, const double *const *wp, const S *const *ep, const S *const *xp,
                                                T (&acc)[DB_TV][DB_TS][DB_TR])
{
    double wk[DB_TV];
    T ev[DB_TS], xv[DB_TR];
#pragma unroll
    for (int v = 0; v < DB_TV; ++v) wk[v] = wp[v][k];
#pragma unroll
    for (int j = 0; j < DB_TR; ++j) xv[j] = emg::widen(xp[j][k]);
#pragma unroll
    for (int i = 0; i < DB_TS; ++i) ev[i] = emg::widen(ep[i][k]);
    dots_block_fma<T>(wk, ev, xv, acc);
}

// T, S, V: as in k_sensitivity_dots. Rows / columns / vectors of a tile past ns / nr / nv repeat the last one (cache
// hits) and are not stored. Workgroup (chunk, group of blockDim.x / 64 tiles); partial[((v * ns + s) * nr + r) * nchunk
// + chunk].
template <class T, class S, int V>
__global__ __launch_bounds__(DB_WAVES * 64) void k_sensitivity_dots_block(size_t n, const S *e, size_t es, int ns, const S *x,
                                                                          size_t xs, int nr, const double *w, size_t wst,
                                                                          int nv, size_t nchunk, T *partial)
{
    const unsigned nst = ((unsigned)ns + DB_TS - 1) / DB_TS, nrt = ((unsigned)nr + DB_TR - 1) / DB_TR;
    const unsigned nvt = ((unsigned)nv + DB_TV - 1) / DB_TV, ntile = nst * nrt * nvt;          // (dots_block_tiles)
    const unsigned waves = blockDim.x >> 6, ngroup = (ntile + waves - 1) / waves;
    const int lane = threadIdx.x & 63;
    const unsigned tile = (blockIdx.x % ngroup) * waves + (threadIdx.x >> 6);
    const size_t chunk = blockIdx.x / ngroup;
    if (tile >= ntile) return;                       // (a whole wave: there is no barrier below)
    const int s0 = (int)(tile % nst) * DB_TS, r0 = (int)(tile / nst % nrt) * DB_TR, v0 = (int)(tile / (nst * nrt)) * DB_TV;
    const S *ep[DB_TS], *xp[DB_TR];
    const double *wp[DB_TV];
#pragma unroll
    for (int i = 0; i < DB_TS; ++i) ep[i] = e + (size_t)min(s0 + i, ns - 1) * es;
#pragma unroll
    for (int j = 0; j < DB_TR; ++j) xp[j] = x + (size_t)min(r0 + j, nr - 1) * xs;
#pragma unroll
    for (int v = 0; v < DB_TV; ++v) wp[v] = w + (size_t)min(v0 + v, nv - 1) * wst;
    T acc[DB_TV][DB_TS][DB_TR];
#pragma unroll
    for (int v = 0; v < DB_TV; ++v)
#pragma unroll
        for (int i = 0; i < DB_TS; ++i)
#pragma unroll
            for (int j = 0; j < DB_TR; ++j) acc[v][i][j] = emg::zero<T>();
    const size_t k0 = chunk * DB_CHUNK;
    const size_t k1 = k0 + DB_CHUNK < n ? k0 + DB_CHUNK : n;
    if constexpr (V == 1) {
        for (size_t kb = k0 + lane; kb < k1; kb += (size_t)64 * DB_UNROLL) {
#pragma unroll
            for (int u = 0; u < DB_UNROLL; ++u) {
                const size_t k = kb + (size_t)u * 64;
                if (k < k1) dots_block_step<T, S>(k, wp, ep, xp, acc);
            }
        }
    } else {
        static_assert(DB_CHUNK % V == 0 && sizeof(S) * V == 16, "a chunk starts on a 16-byte boundary of every row");
        // (a pack is V consecutive k in flight already: no further unrolling, which would spill)
        for (size_t k = k0 + (size_t)lane * V; k < k1; k += (size_t)64 * V) {
            if (k + V <= k1) {
                Pack<double, V> wv[DB_TV];
                Pack<S, V> xv[DB_TR], ev[DB_TS];
#pragma unroll
                for (int v = 0; v < DB_TV; ++v) wv[v] = load_pack<double, V>(wp[v] + k);
#pragma unroll
                for (int j = 0; j < DB_TR; ++j) xv[j] = load_pack<S, V>(xp[j] + k);
#pragma unroll
                for (int i = 0; i < DB_TS; ++i) ev[i] = load_pack<S, V>(ep[i] + k);
#pragma unroll
                for (int m = 0; m < V; ++m) {
                    double wk[DB_TV];
                    T em[DB_TS], xm[DB_TR];
#pragma unroll
                    for (int v = 0; v < DB_TV; ++v) wk[v] = wv[v].v[m];
#pragma unroll
                    for (int j = 0; j < DB_TR; ++j) xm[j] = emg::widen(xv[j].v[m]);
#pragma unroll
                    for (int i = 0; i < DB_TS; ++i) em[i] = emg::widen(ev[i].v[m]);
                    dots_block_fma<T>(wk, em, xm, acc);
                }
            } else {
                for (size_t kk = k; kk < k1; ++kk) dots_block_step<T, S>(kk, wp, ep, xp, acc);
            }
        }
    }
#pragma unroll
    for (int v = 0; v < DB_TV; ++v)
#pragma unroll
        for (int i = 0; i < DB_TS; ++i)
#pragma unroll
            for (int j = 0; j < DB_TR; ++j) {
                T a = acc[v][i][j];
                for (int off = 32; off > 0; off >>= 1) a += shfl_down_t(a, off);
                if (lane == 0 && v0 + v < nv && s0 + i < ns && r0 + j < nr)
                    partial[(((size_t)(v0 + v) * ns + s0 + i) * nr + r0 + j) * nchunk + chunk] = a;
            }
}

// ---- combine_block. One thread per k (V > 1: per V consecutive k): its first CMB_XR receiver values stay in
// registers, every e_s[k] is loaded once and used for the CB_TV vectors of the tile (blockIdx.y). Per vector the
// operations are combine_one's, term by term -- r ascending into u, then sum = e_s u + sum, s ascending --, so row v of
// t is the bits of k_sensitivity_combine with coef[v], for either load width. Only the sums of the vectors stay live
// over s (u is per vector; receivers beyond CMB_XR are read again per source AND vector: cache hits). Vectors of a
// tile past nv are skipped (the branch is uniform). The coefficients are uniform over the wave.
constexpr int CB_TV = 8;

template <class T, class S, int V>
__global__ __launch_bounds__(256) void k_sensitivity_combine_block(size_t n, const S *__restrict__ e, size_t es, int ns,
                                                                   const S *__restrict__ x, size_t xs, int nr,
                                                                   const T *__restrict__ coef, int nv, T *__restrict__ t,
                                                                   size_t ts)
{
    const size_t k = ((size_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (k >= n) return;
    const int v0 = blockIdx.y * CB_TV, nvt = min(CB_TV, nv - v0);
    const size_t cvs = (size_t)ns * nr;
    coef += (size_t)v0 * cvs;
    t += (size_t)v0 * ts;
    if constexpr (V > 1) {
        static_assert(sizeof(S) * V == 16, "one 16-byte load per field");
        if (k + V <= n) {
            Pack<S, V> xv[CMB_XR];
#pragma unroll
            for (int j = 0; j < CMB_XR; ++j) xv[j] = load_pack<S, V>(x + (size_t)min(j, nr - 1) * xs + k);
            Pack<T, V> sum[CB_TV];
#pragma unroll
            for (int v = 0; v < CB_TV; ++v)
#pragma unroll
                for (int m = 0; m < V; ++m) sum[v].v[m] = emg::zero<T>();
            for (int s = 0; s < ns; ++s) {
                const Pack<S, V> ev = load_pack<S, V>(e + (size_t)s * es + k);
#pragma unroll
                for (int v = 0; v < CB_TV; ++v)
                    if (v < nvt) {
                        const T *c = coef + (size_t)v * cvs + (size_t)s * nr;
                        T u[V];
#pragma unroll
                        for (int m = 0; m < V; ++m) u[m] = emg::zero<T>();
#pragma unroll
                        for (int j = 0; j < CMB_XR; ++j)
                            if (j < nr) {
#pragma unroll
                                for (int m = 0; m < V; ++m) u[m] = emg::mad(c[j], emg::widen(xv[j].v[m]), u[m]);
                            }
                        for (int r = CMB_XR; r < nr; ++r) {
                            const Pack<S, V> xr = load_pack<S, V>(x + (size_t)r * xs + k);
#pragma unroll
                            for (int m = 0; m < V; ++m) u[m] = emg::mad(c[r], emg::widen(xr.v[m]), u[m]);
                        }
#pragma unroll
                        for (int m = 0; m < V; ++m) sum[v].v[m] = emg::mad(emg::widen(ev.v[m]), u[m], sum[v].v[m]);
                    }
            }
#pragma unroll
            for (int v = 0; v < CB_TV; ++v)
                if (v < nvt) *reinterpret_cast<Pack<T, V> *>(t + (size_t)v * ts + k) = sum[v];
            return;
        }
    }
    // element by element: V = 1, or the last thread of an n that is no multiple of V
    const size_t kend = k + V < n ? k + V : n;
    for (size_t kk = k; kk < kend; ++kk) {
        T xv[CMB_XR];
#pragma unroll
        for (int j = 0; j < CMB_XR; ++j) xv[j] = emg::widen(x[(size_t)min(j, nr - 1) * xs + kk]);
        T sum[CB_TV];
#pragma unroll
        for (int v = 0; v < CB_TV; ++v) sum[v] = emg::zero<T>();
        for (int s = 0; s < ns; ++s) {
            const T ev = emg::widen(e[(size_t)s * es + kk]);
#pragma unroll
            for (int v = 0; v < CB_TV; ++v)
                if (v < nvt) {
                    const T *c = coef + (size_t)v * cvs + (size_t)s * nr;
                    T u = emg::zero<T>();
#pragma unroll
                    for (int j = 0; j < CMB_XR; ++j)
                        if (j < nr) u = emg::mad(c[j], xv[j], u);
                    for (int r = CMB_XR; r < nr; ++r) u = emg::mad(c[r], emg::widen(x[(size_t)r * xs + kk]), u);
                    sum[v] = emg::mad(ev, u, sum[v]);
                }
        }
#pragma unroll
        for (int v = 0; v < CB_TV; ++v)
            if (v < nvt) t[(size_t)v * ts + kk] = sum[v];
    }
}

inline size_t dots_block_chunks(size_t n) { return (n + DB_CHUNK - 1) / DB_CHUNK; }
inline size_t tiles_of(int count, int tile) { return ((size_t)count + tile - 1) / tile; }

inline size_t dots_block_tiles(int ns, int nr, int nv)
{
    return tiles_of(ns, DB_TS) * tiles_of(nr, DB_TR) * tiles_of(nv, DB_TV);
}

// Waves (= tiles) per workgroup and workgroups per chunk: functions of the sizes alone.
inline unsigned dots_block_waves(size_t ntile) { return (unsigned)(ntile < (size_t)DB_WAVES ? ntile : (size_t)DB_WAVES); }
inline size_t dots_block_groups(size_t ntile) { return (ntile + dots_block_waves(ntile) - 1) / dots_block_waves(ntile); }

template <class T, class S, int V>
int launch_dots_block_as(size_t n, const void *e, size_t es, int ns, const void *x, size_t xs, int nr, const double *w,
                         size_t wst, int nv, T scale, void *out, double *ws, hipStream_t st)
{
    const size_t nchunk = dots_block_chunks(n), ntile = dots_block_tiles(ns, nr, nv);
    const dim3 grid((unsigned)(nchunk * dots_block_groups(ntile)));
    hipLaunchKernelGGL((k_sensitivity_dots_block<T, S, V>), grid, dim3(64 * dots_block_waves(ntile)), 0, st, n, (const S *)e, es,
                       ns, (const S *)x, xs, nr, w, wst, nv, nchunk, (T *)ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sensitivity_dots_final<T>, dim3((unsigned)((size_t)nv * ns * nr)), dim3(256), 0, st, (const T *)ws,
                       nchunk, scale, (T *)out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Narrow stacks: 16-byte loads where every row of both stacks and of w starts on a 16-byte boundary.
template <class T, class S>
int launch_dots_block(size_t n, const void *e, size_t es, int ns, const void *x, size_t xs, int nr, const double *w,
                      size_t wst, int nv, T scale, void *out, double *ws, hipStream_t st)
{
    if (nv == 1)                                     // one vector: the 4 x 4 tile of k_sensitivity_dots (ws is large enough)
        return launch_dots<T, S>(n, e, es, ns, x, xs, nr, w, scale, out, ws, st);
    if constexpr (sizeof(S) < sizeof(T)) {
        if (rows_on_16_bytes<S>(e, es) && rows_on_16_bytes<S>(x, xs) && rows_on_16_bytes<double>(w, wst))
            return launch_dots_block_as<T, S, (int)(16 / sizeof(S))>(n, e, es, ns, x, xs, nr, w, wst, nv, scale, out, ws, st);
    }
    return launch_dots_block_as<T, S, 1>(n, e, es, ns, x, xs, nr, w, wst, nv, scale, out, ws, st);
}

template <class T, class S>
int launch_combine_block(size_t n, const void *e, size_t es, int ns, const void *x, size_t xs, int nr, const void *coef,
                         int nv, void *t, size_t ts, hipStream_t st)
{
    if (nv == 1)                                     // one vector: k_sensitivity_combine, the same bits
        return launch_combine<T, S>(n, e, es, ns, x, xs, nr, coef, t, st);
    const unsigned nvt = (unsigned)tiles_of(nv, CB_TV);
    if constexpr (sizeof(S) < sizeof(T)) {
        if (rows_on_16_bytes<S>(e, es) && rows_on_16_bytes<S>(x, xs) && rows_on_16_bytes<T>(t, ts)) {
            constexpr int V = (int)(16 / sizeof(S));
            const size_t nblk = ((n + V - 1) / V + 255) / 256;
            hipLaunchKernelGGL((k_sensitivity_combine_block<T, S, V>), dim3((unsigned)nblk, nvt), dim3(256), 0, st, n,
                               (const S *)e, es, ns, (const S *)x, xs, nr, (const T *)coef, nv, (T *)t, ts);
            HIP_TRY(hipGetLastError());
            return 0;
        }
    }
    hipLaunchKernelGGL((k_sensitivity_combine_block<T, S, 1>), dim3((unsigned)((n + 255) / 256), nvt), dim3(256), 0, st, n,
                       (const S *)e, es, ns, (const S *)x, xs, nr, (const T *)coef, nv, (T *)t, ts);
    HIP_TRY(hipGetLastError());
    return 0;
}

inline bool dots_block_fits(size_t n, int ns, int nr, int nv)
{
    return (size_t)nv * (size_t)ns <= 0x7fffffffu / (size_t)nr &&
           dots_block_chunks(n) <= 0x7fffffffu / dots_block_groups(dots_block_tiles(ns, nr, nv)) &&
           tiles_of(ns, DOT_TS) <= 65535 && tiles_of(nr, DOT_TR) <= 65535;          // (nv = 1 runs k_sensitivity_dots)
}

// The checks of emg3d_dev_sensitivity_dots_block / _combine_block and of their _sp siblings.
template <bool SP>
int sensitivity_dots_block(size_t n, int is_complex, const void *e, size_t e_stride, int ns, const void *x, size_t x_stride,
                           int nr, const double *w, size_t w_stride, int nv, double scale_re, double scale_im, void *out,
                           double *ws, size_t ws_len, void *stream)
{
    if (n < 1 || ns < 1 || nr < 1 || nv < 1 || !e || !x || !w || !out || !ws || e_stride < n || x_stride < n || w_stride < n)
        return fail(EMG3D_ERR_BADARG, "sensitivity_dots_block: bad argument");
    if (!dots_block_fits(n, ns, nr, nv))
        return fail(EMG3D_ERR_BADARG, "sensitivity_dots_block: too large for one launch");
    if (ws_len < 2 * (size_t)nv * (size_t)ns * (size_t)nr * dots_block_chunks(n))
        return fail(EMG3D_ERR_BADARG, "sensitivity_dots_block: workspace too small (emg3d_sensitivity_dots_block_ws_len)");
    using C = std::conditional_t<SP, emg::cplxf, cplx>;
    using R = std::conditional_t<SP, float, double>;
    return is_complex ? launch_dots_block<cplx, C>(n, e, e_stride, ns, x, x_stride, nr, w, w_stride, nv,
                                                   cplx(scale_re, scale_im), out, ws, (hipStream_t)stream)
                      : launch_dots_block<double, R>(n, e, e_stride, ns, x, x_stride, nr, w, w_stride, nv, scale_re, out, ws,
                                                     (hipStream_t)stream);
}

template <bool SP>
int sensitivity_combine_block(size_t n, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                              size_t x_stride, int nr, const void *coef, int nv, void *t, size_t t_stride, void *stream)
{
    if (n < 1 || ns < 1 || nr < 1 || nv < 1 || !e || !x || !coef || !t || e_stride < n || x_stride < n || t_stride < n)
        return fail(EMG3D_ERR_BADARG, "sensitivity_combine_block: bad argument");
    if ((n + 255) / 256 > 0x7fffffffu || tiles_of(nv, CB_TV) > 65535)
        return fail(EMG3D_ERR_BADARG, "sensitivity_combine_block: too large for one launch");
    using C = std::conditional_t<SP, emg::cplxf, cplx>;
    using R = std::conditional_t<SP, float, double>;
    return is_complex ? launch_combine_block<cplx, C>(n, e, e_stride, ns, x, x_stride, nr, coef, nv, t, t_stride,
                                                      (hipStream_t)stream)
                      : launch_combine_block<double, R>(n, e, e_stride, ns, x, x_stride, nr, coef, nv, t, t_stride,
                                                        (hipStream_t)stream);
}

}  // namespace

extern "C" {

size_t emg3d_sensitivity_dots_block_ws_len(int ns, int nr, int nv, size_t n)
{
    if (ns < 1 || nr < 1 || nv < 1 || n < 1) return 0;
    return 2 * (size_t)nv * (size_t)ns * (size_t)nr * dots_block_chunks(n);
}

int emg3d_dev_sensitivity_dots_block(size_t n, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                                     size_t x_stride, int nr, const double *w, size_t w_stride, int nv, double scale_re,
                                     double scale_im, void *out, double *ws, size_t ws_len, void *stream)
{
    return sensitivity_dots_block<false>(n, is_complex, e, e_stride, ns, x, x_stride, nr, w, w_stride, nv, scale_re, scale_im,
                                         out, ws, ws_len, stream);
}

int emg3d_dev_sensitivity_dots_block_sp(size_t n, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                                        size_t x_stride, int nr, const double *w, size_t w_stride, int nv, double scale_re,
                                        double scale_im, void *out, double *ws, size_t ws_len, void *stream)
{
    return sensitivity_dots_block<true>(n, is_complex, e, e_stride, ns, x, x_stride, nr, w, w_stride, nv, scale_re, scale_im,
                                        out, ws, ws_len, stream);
}

int emg3d_dev_sensitivity_combine_block(size_t n, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                                        size_t x_stride, int nr, const void *coef, int nv, void *t, size_t t_stride,
                                        void *stream)
{
    return sensitivity_combine_block<false>(n, is_complex, e, e_stride, ns, x, x_stride, nr, coef, nv, t, t_stride, stream);
}

int emg3d_dev_sensitivity_combine_block_sp(size_t n, int is_complex, const void *e, size_t e_stride, int ns, const void *x,
                                           size_t x_stride, int nr, const void *coef, int nv, void *t, size_t t_stride,
                                           void *stream)
{
    return sensitivity_combine_block<true>(n, is_complex, e, e_stride, ns, x, x_stride, nr, coef, nv, t, t_stride, stream);
}

}  // extern "C"
