// correlators.hip -- the two-point functions Spin_Spin and Vortex_Vortex of both formulations on the device.
//
// Direct pair (Villain Spin_Spin, spin.py:28-42; Worldline Vortex_Vortex, vortex.py:22-37): one cross-correlation
//   C(r) = 1/V sum_x conj f(x) f(x - r)   (lattice/compact.py:465-..., there FFT-accelerated through np.fft)
// of a unit-modulus field formed from the resident configuration.  Two paths: a hand-written radix-2 row FFT in LDS
// (N a power of two, 4 <= N <= 4096; row FFT, tiled transpose, row FFT, twice, with the field formation, |F|^2 and
// the 1/V^2 scale fused into the loads and the last store) and a tiled direct sum (any N with V <= 2^16).
//
// Taxicab pair (Worldline Spin_Spin, spin.py:50-224; Villain Vortex_Vortex, vortex.py:63-189): the reference
// gathers, for every displacement and every origin, the links of a fixed time-then-space path.  A periodic run of
// links is a difference of two entries of the prefix sums over the doubled row or column, so the measurement is
// O(V) prefix entries and one exp per (displacement, origin):
//   out[dt, dx] = 1/V sum_(t0, x0) exp(a s + b (|dt| + |dx|)),
//   s = (Pt[x0][bt + dt] - Pt[x0][bt]) + xsign (Px[t0 + dt][bx + dx] - Px[t0 + dt][bx]),
// bt = t0 + off (+ N when dt < 0), bx = x0 + off (+ N when dx < 0); (tcomp, xcomp, off, xsign) = (0, 1, 0, +1) for the
// Worldline path and (1, 0, 1, -1) for the Villain dual path.
//
// Every sum has a fixed order that depends on N alone: no atomics, and no dependence on the launch geometry.
#include <cmath>
#include <mutex>
#include <type_traits>

#include "common.h"

namespace {

constexpr double TWO_PI = 6.283185307179586;  // 2 * np.pi
constexpr int FFT_MIN = 4, FFT_MAX = 4096;
constexpr int64_t DIRECT_MAX_V = 65536;
constexpr int TAXI_MAX_N = 2048;  // the kernel's LDS rows: (3 N + 1) 8-byte words
constexpr int TAXI_UNITS = 16;    // the origin rows are summed in about this many units (fixed by N)

enum FieldMode {
    F_COMPLEX = 0,
    F_PHI = 1,
    F_VINT = 2,
    F_VFLOAT = 3,
    F_POWER = 4,
    F_POWER_PAIR = 5,  // the spectrum of z = a + i b, unpacked: |A|^2 + i |B|^2
    F_PLANAR = 6,      // two real fields, p[i] + i p[V + i]
    F_VILLAIN_AW = 7,  // the action density and d(n) of a Villain state (p = phi, q = n)
    F_WORLDLINE_AW = 8,        // 1 - l^2 / (2 kappa) and d(l) of a Worldline state (p = m, q = v int64)
    F_WORLDLINE_AW_EXACT = 9,  // the same from the exact integers W l, d(W l)
    F_WORLDLINE_AW_VFLOAT = 10  // the same with float v
};

// What a kernel loads site i of its input field from: a complex field, phi (exp(i phi), spin.py:40), v
// (exp(2 pi i v / W), vortex.py:35: NumPy's complex / real multiplies by 1 / W), a spectrum (|F|^2), or the packed
// pair of real fields z = a + i b of the action and winding two-point functions (action.py:64-152, winding.py:76-202).
struct FieldSrc {
    const void *p;
    int mode;
    double winv;
    const void *q = nullptr;
    int N = 0;
    double coef = 0.0;  // kappa / 2 (Villain), 1 / (2 kappa) (Worldline)
    double W = 1.0;
    int64_t Wi = 1;
};

// Links.Villain at (t, x), the arithmetic of villain_links
__device__ __forceinline__ double villain_link(const double *__restrict__ phi, const int64_t *__restrict__ n, int N,
                                               int comp, int t, int x) {
    const int64_t V = (int64_t)N * N, s = (int64_t)t * N + x;
    const int64_t f = comp == 0 ? (int64_t)(t + 1 == N ? 0 : t + 1) * N + x : (int64_t)t * N + (x + 1 == N ? 0 : x + 1);
    return (phi[f] - phi[s]) - TWO_PI * (double)n[(int64_t)comp * V + s];
}

// a = kappa / 2 (l_0^2 + l_1^2) (action.py:90) and b = d(n) = (n_1[t+1] - n_1) - (n_0[x+1] - n_0) (winding.py:85)
__device__ __forceinline__ double2 villain_aw(const FieldSrc &S, int64_t i) {
    const double *phi = (const double *)S.p;
    const int64_t *n = (const int64_t *)S.q;
    const int N = S.N, t = (int)(i / N), x = (int)(i - (int64_t)t * N);
    const int64_t V = (int64_t)N * N;
    const int64_t ft = (int64_t)(t + 1 == N ? 0 : t + 1) * N + x, fx = (int64_t)t * N + (x + 1 == N ? 0 : x + 1);
    const double l0 = villain_link(phi, n, N, 0, t, x), l1 = villain_link(phi, n, N, 1, t, x);
    const int64_t dn = (n[V + ft] - n[V + i]) - (n[fx] - n[i]);
    return make_double2(S.coef * (l0 * l0 + l1 * l1), (double)dn);
}

// Links.Worldline at (t, x), the arithmetic of worldline_links: T = int64_t gives W l = W m - delta(v)
template <typename TV, typename T>
__device__ __forceinline__ T worldline_link(const int64_t *__restrict__ m, const TV *__restrict__ v, int N, int comp,
                                            int t, int x, double W, int64_t Wi) {
    const int64_t V = (int64_t)N * N, s = (int64_t)t * N + x;
    TV dl;
    if (comp == 0)
        dl = v[s] - v[(int64_t)t * N + (x == 0 ? N - 1 : x - 1)];
    else
        dl = -(v[s] - v[(int64_t)(t == 0 ? N - 1 : t - 1) * N + x]);
    if (std::is_integral<T>::value) return (T)(Wi * m[(int64_t)comp * V + s] - (int64_t)dl);
    return (T)((double)m[(int64_t)comp * V + s] - (double)dl / W);
}

// (l_0^2 + l_1^2, d(l)) of site i, or the same of W l as integers; d(l) = (l_1[t+1] - l_1) - (l_0[x+1] - l_0)
template <typename TV, typename T>
__device__ __forceinline__ void worldline_site(const int64_t *__restrict__ m, const TV *__restrict__ v, int N,
                                               int64_t i, double W, int64_t Wi, T *l2, T *dl) {
    const int t = (int)(i / N), x = (int)(i - (int64_t)t * N);
    const int tp = t + 1 == N ? 0 : t + 1, xp = x + 1 == N ? 0 : x + 1;
    const T l0 = worldline_link<TV, T>(m, v, N, 0, t, x, W, Wi), l1 = worldline_link<TV, T>(m, v, N, 1, t, x, W, Wi);
    const T l1t = worldline_link<TV, T>(m, v, N, 1, tp, x, W, Wi), l0x = worldline_link<TV, T>(m, v, N, 0, t, xp, W, Wi);
    *l2 = l0 * l0 + l1 * l1;
    *dl = (l1t - l1) - (l0x - l0);
}

// a = 1 - (l_0^2 + l_1^2) / (2 kappa) (action.py:136-140) and b = d(l) (winding.py:182)
template <typename TV, bool EXACT>
__device__ __forceinline__ double2 worldline_aw(const FieldSrc &S, int64_t i) {
    if (EXACT) {
        int64_t l2, dl;
        worldline_site<TV, int64_t>((const int64_t *)S.p, (const TV *)S.q, S.N, i, S.W, S.Wi, &l2, &dl);
        return make_double2(1.0 - S.coef * ((double)l2 / (S.W * S.W)), (double)dl / S.W);
    }
    double l2, dl;
    worldline_site<TV, double>((const int64_t *)S.p, (const TV *)S.q, S.N, i, S.W, S.Wi, &l2, &dl);
    return make_double2(1.0 - S.coef * l2, dl);
}

__device__ __forceinline__ double2 load_field(const FieldSrc &S, int64_t i) {
    double ang;
    switch (S.mode) {
        case F_COMPLEX:
            return ((const double2 *)S.p)[i];
        case F_POWER: {
            const double2 z = ((const double2 *)S.p)[i];
            return make_double2(z.x * z.x + z.y * z.y, 0.0);
        }
        case F_POWER_PAIR: {
            // Z(-k) of element [r][c] sits at [(N - r) % N][(N - c) % N], in the transposed layout too
            const int N = S.N, r = (int)(i / N), c = (int)(i - (int64_t)r * N);
            const double2 z = ((const double2 *)S.p)[i];
            const double2 w = ((const double2 *)S.p)[(int64_t)(r == 0 ? 0 : N - r) * N + (c == 0 ? 0 : N - c)];
            // A = (Z + conj Z(-k)) / 2, B = (Z - conj Z(-k)) / (2i)
            const double ar = z.x + w.x, ai = z.y - w.y, br = z.x - w.x, bi = z.y + w.y;
            return make_double2(0.25 * (ar * ar + ai * ai), 0.25 * (br * br + bi * bi));
        }
        case F_PLANAR:
            return make_double2(((const double *)S.p)[i], ((const double *)S.p)[(int64_t)S.N * S.N + i]);
        case F_VILLAIN_AW:
            return villain_aw(S, i);
        case F_WORLDLINE_AW:
            return worldline_aw<int64_t, false>(S, i);
        case F_WORLDLINE_AW_EXACT:
            return worldline_aw<int64_t, true>(S, i);
        case F_WORLDLINE_AW_VFLOAT:
            return worldline_aw<double, false>(S, i);
        case F_PHI:
            ang = ((const double *)S.p)[i];
            break;
        case F_VINT:
            ang = (TWO_PI * (double)((const int64_t *)S.p)[i]) * S.winv;
            break;
        default:
            ang = (TWO_PI * ((const double *)S.p)[i]) * S.winv;
            break;
    }
    double s, c;
    sincos(ang, &s, &c);
    return make_double2(c, s);
}

__global__ void form_field(FieldSrc src, double2 *dst, int64_t V) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < V) dst[i] = load_field(src, i);
}

// One forward DFT per row (e^{-2 pi i k x / N}), in place in LDS: bit-reversed load, log2 N radix-2 stages.  `tpr`
// threads work on a row and a workgroup holds blockDim.x / tpr rows; tw[k] = e^{-2 pi i k / N}, k < N / 2.  The store
// scales the real part by `scale` and the imaginary part by `scale_im`; planar: the two parts go to two real N x N
// arrays, dst and dst + V doubles (the two correlators of a packed pair).
__global__ void fft_rows(FieldSrc src, double2 *dst, const double2 *__restrict__ tw, int N, int logN, int tpr,
                         double scale, double scale_im, int planar) {
    extern __shared__ double2 fft_lds[];
    const int lr = threadIdx.x / tpr, lt = threadIdx.x % tpr;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x / tpr) + lr;
    const bool live = row < N;
    double2 *x = fft_lds + (size_t)lr * N;
    if (live)
        for (int i = lt; i < N; i += tpr) x[__brev((unsigned)i) >> (32 - logN)] = load_field(src, row * N + i);
    __syncthreads();
    for (int s = 0; s < logN; s++) {
        const int half = 1 << s;
        if (live)
            for (int j = lt; j < N / 2; j += tpr) {
                const int k = j & (half - 1);
                const int i0 = ((j >> s) << (s + 1)) + k, i1 = i0 + half;
                const double2 w = tw[(size_t)k << (logN - 1 - s)];
                const double2 a = x[i0], b = x[i1];
                const double tr = w.x * b.x - w.y * b.y, ti = w.x * b.y + w.y * b.x;
                x[i0] = make_double2(a.x + tr, a.y + ti);
                x[i1] = make_double2(a.x - tr, a.y - ti);
            }
        __syncthreads();
    }
    if (live && !planar)
        for (int i = lt; i < N; i += tpr) dst[row * N + i] = make_double2(x[i].x * scale, x[i].y * scale_im);
    if (live && planar) {
        double *re = (double *)dst, *im = re + (int64_t)N * N;
        for (int i = lt; i < N; i += tpr) {
            re[row * N + i] = x[i].x * scale;
            im[row * N + i] = x[i].y * scale_im;
        }
    }
}

// out[c][r] = in[r][c], 32 x 32 tiles through LDS (block 32 x 8)
__global__ void transpose_complex(const double2 *__restrict__ in, double2 *__restrict__ out, int N) {
    __shared__ double2 tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += 8) {
        const int r = by + j, c = bx + threadIdx.x;
        if (r < N && c < N) tile[j][threadIdx.x] = in[(size_t)r * N + c];
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += 8) {
        const int r = bx + j, c = by + threadIdx.x;
        if (r < N && c < N) out[(size_t)r * N + c] = tile[threadIdx.x][j];
    }
}

// The definition, summed directly: workgroup = (dt, tile of dx), lanes over dx.  Per t it stages row t of f and the
// doubled row t - dt; a lane sums its row in x order and adds the row sums in t order.
__global__ void correlation_direct(const double2 *__restrict__ f, double2 *__restrict__ out, int N) {
    extern __shared__ double2 dir_lds[];
    double2 *frow = dir_lds, *g = dir_lds + N;  // g: 2 N
    const int rt = blockIdx.x, rx = blockIdx.y * blockDim.x + threadIdx.x;
    double tr = 0.0, ti = 0.0;
    for (int t = 0; t < N; t++) {
        const int tg = t - rt < 0 ? t - rt + N : t - rt;
        __syncthreads();
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
            frow[i] = f[(size_t)t * N + i];
            const double2 z = f[(size_t)tg * N + i];
            g[i] = z;
            g[i + N] = z;
        }
        __syncthreads();
        if (rx < N) {
            double rr = 0.0, ri = 0.0;
            for (int x = 0; x < N; x++) {
                const double2 a = frow[x], b = g[x - rx + N];  // f(t - dt, x - dx)
                rr += a.x * b.x + a.y * b.y;
                ri += a.x * b.y - a.y * b.x;
            }
            tr += rr;
            ti += ri;
        }
    }
    const double V = (double)N * (double)N;
    if (rx < N) out[(size_t)rt * N + rx] = make_double2(tr / V, ti / V);
}

// The same for the two real fields packed as f = a + i b: C_aa(r) = 1/V sum_x a(x) a(x - r) and C_bb, each with the
// sums of correlation_direct, stored scaled to two real N x N arrays (out, out + V).
__global__ void correlation_direct_real(const double2 *__restrict__ f, double *__restrict__ out, int N, double scale_aa,
                                        double scale_bb) {
    extern __shared__ double2 dir_lds[];
    double2 *frow = dir_lds, *g = dir_lds + N;  // g: 2 N
    const int rt = blockIdx.x, rx = blockIdx.y * blockDim.x + threadIdx.x;
    double ta = 0.0, tb = 0.0;
    for (int t = 0; t < N; t++) {
        const int tg = t - rt < 0 ? t - rt + N : t - rt;
        __syncthreads();
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
            frow[i] = f[(size_t)t * N + i];
            const double2 z = f[(size_t)tg * N + i];
            g[i] = z;
            g[i + N] = z;
        }
        __syncthreads();
        if (rx < N) {
            double ra = 0.0, rb = 0.0;
            for (int x = 0; x < N; x++) {
                const double2 a = frow[x], b = g[x - rx + N];
                ra += a.x * b.x;
                rb += a.y * b.y;
            }
            ta += ra;
            tb += rb;
        }
    }
    const double V = (double)N * (double)N;
    if (rx < N) {
        out[(size_t)rt * N + rx] = (ta / V) * scale_aa;
        out[(size_t)N * N + (size_t)rt * N + rx] = (tb / V) * scale_bb;
    }
}

// ---- the Worldline sums (sv_worldline_sums) -------------------------------------------------------------------------
// A workgroup sums SUM_SITES consecutive sites: a thread its own in index order, then a tree over the threads, so
// the float sums have an order fixed by N; the integer sums are exact.  The host adds the workgroups' words in order.
constexpr int SUM_THREADS = 256, SUM_SITES = 4096;
struct SumWords {
    double l2, dl2;
    int64_t m0, m1, wl2, wdl2;
};

template <typename TV, bool EXACT>
__global__ void worldline_sums(const int64_t *__restrict__ m, const TV *__restrict__ v, int N, double W, int64_t Wi,
                               SumWords *partial) {
    __shared__ SumWords red[SUM_THREADS];
    const int64_t V = (int64_t)N * N, base = (int64_t)blockIdx.x * SUM_SITES;
    SumWords w = {0.0, 0.0, 0, 0, 0, 0};
    for (int k = 0; k < SUM_SITES / SUM_THREADS; k++) {
        const int64_t i = base + (int64_t)k * SUM_THREADS + threadIdx.x;
        if (i >= V) break;
        if (EXACT) {
            int64_t l2, dl;
            worldline_site<TV, int64_t>(m, v, N, i, W, Wi, &l2, &dl);
            w.wl2 += l2;
            w.wdl2 += dl * dl;
        } else {
            double l2, dl;
            worldline_site<TV, double>(m, v, N, i, W, Wi, &l2, &dl);
            w.l2 += l2;
            w.dl2 += dl * dl;
        }
        w.m0 += m[i];
        w.m1 += m[V + i];
    }
    red[threadIdx.x] = w;
    __syncthreads();
    for (int h = SUM_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            SumWords &a = red[threadIdx.x];
            const SumWords b = red[threadIdx.x + h];
            a.l2 += b.l2;
            a.dl2 += b.dl2;
            a.m0 += b.m0;
            a.m1 += b.m1;
            a.wl2 += b.wl2;
            a.wdl2 += b.wdl2;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// ---- links of the resident states ------------------------------------------------------------------------------
// Links.Villain (links.py:17-31): d(phi) - 2 pi n
__global__ void villain_links(const double *__restrict__ phi, const int64_t *__restrict__ n, double *links, int N) {
    const int64_t V = (int64_t)N * N, s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= V) return;
    const int t = (int)(s / N), x = (int)(s % N);
    const int64_t st = (int64_t)(t + 1 == N ? 0 : t + 1) * N + x, sx = (int64_t)t * N + (x + 1 == N ? 0 : x + 1);
    links[s] = (phi[st] - phi[s]) - TWO_PI * (double)n[s];
    links[V + s] = (phi[sx] - phi[s]) - TWO_PI * (double)n[V + s];
}

// Links.Worldline (links.py:35-45): m - delta(v) / W, delta(v)_0 = v[t, x] - v[t, x - 1], delta(v)_1 = -(v[t, x] -
// v[t - 1, x]).  EXACT (integer v, integer W): W m - delta(v) as int64, the taxicab sums divide once.
template <typename TV, bool EXACT>
__global__ void worldline_links(const int64_t *__restrict__ m, const TV *__restrict__ v, void *links, int N, double W,
                                int64_t Wi) {
    const int64_t V = (int64_t)N * N, s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= V) return;
    const int t = (int)(s / N), x = (int)(s % N);
    const int64_t sx = (int64_t)t * N + (x == 0 ? N - 1 : x - 1), st = (int64_t)(t == 0 ? N - 1 : t - 1) * N + x;
    const TV d0 = v[s] - v[sx], d1 = -(v[s] - v[st]);
    if (EXACT) {
        ((int64_t *)links)[s] = Wi * m[s] - (int64_t)d0;
        ((int64_t *)links)[V + s] = Wi * m[V + s] - (int64_t)d1;
    } else {
        ((double *)links)[s] = (double)m[s] - (double)d0 / W;
        ((double *)links)[V + s] = (double)m[V + s] - (double)d1 / W;
    }
}

// ---- taxicab reweighting -----------------------------------------------------------------------------------------
// Prefix sums over the doubled column (Pt, stored (2 N + 1, N)) and the doubled row (Px, stored (N, 2 N + 1)), each
// a sequential sum from 0 (what np.cumsum does): one thread per column / row.
template <typename T>
__global__ void taxicab_prefix(const T *__restrict__ links, T *Pt, T *Px, int N, int tcomp, int xcomp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const T *Lt = links + (size_t)tcomp * N * N, *Lx = links + (size_t)xcomp * N * N;
    T acc = 0;
    Pt[i] = 0;
    for (int j = 0; j < 2 * N; j++) {
        acc += Lt[(size_t)(j < N ? j : j - N) * N + i];
        Pt[(size_t)(j + 1) * N + i] = acc;
    }
    acc = 0;
    T *row = Px + (size_t)i * (2 * N + 1);
    row[0] = 0;
    for (int j = 0; j < 2 * N; j++) {
        acc += Lx[(size_t)i * N + (j < N ? j : j - N)];
        row[j + 1] = acc;
    }
}

__device__ __forceinline__ double taxi_s(double tp, double sx, int xsign, double) { return tp + (double)xsign * sx; }
__device__ __forceinline__ double taxi_s(int64_t tp, int64_t sx, int xsign, double W) {
    return (double)(tp + xsign * sx) / W;
}

// Workgroup = (dt, tile of dx, group of origin units), lanes over dx.  Per origin row t0 the LDS holds the time
// part of every column x0 and the doubled space prefix of row t0 + dt; lane dx reads px[x0 + off + dx] (stride 1
// over the lanes) and px[bx] (two addresses per wave).  A unit is `unit_rows` origin rows, summed in (t0, x0)
// order into partial[unit][dt][dx]; how many units a workgroup takes does not change any sum.
template <typename T>
__global__ void taxicab_sum(const T *__restrict__ Pt, const T *__restrict__ Px, double *partial, int N, int off,
                            int xsign, double a, double b, double W, int unit_rows, int nunits, int units_per_group) {
    extern __shared__ unsigned char taxi_lds[];
    T *tp = (T *)taxi_lds, *px = tp + N;  // N, 2 N + 1
    const int dti = blockIdx.x, dt = dti <= N / 2 ? dti : dti - N;
    const int dxi = blockIdx.y * blockDim.x + threadIdx.x, dx = dxi <= N / 2 ? dxi : dxi - N;
    const bool live = dxi < N;
    const double bl = b * (double)((dt < 0 ? -dt : dt) + (dx < 0 ? -dx : dx));
    const int bt = off + (dt < 0 ? N : 0), bx = off + (dx < 0 ? N : 0);
    const int row_len = 2 * N + 1;
    const int u1 = min(nunits, ((int)blockIdx.z + 1) * units_per_group);
    for (int u = blockIdx.z * units_per_group; u < u1; u++) {
        double acc = 0.0;
        const int t1 = min(N, (u + 1) * unit_rows);
        for (int t0 = u * unit_rows; t0 < t1; t0++) {
            int r = t0 + dt;
            r = r < 0 ? r + N : (r >= N ? r - N : r);
            __syncthreads();
            for (int i = threadIdx.x; i < N; i += blockDim.x)
                tp[i] = Pt[(size_t)(t0 + bt + dt) * N + i] - Pt[(size_t)(t0 + bt) * N + i];
            for (int i = threadIdx.x; i < row_len; i += blockDim.x) px[i] = Px[(size_t)r * row_len + i];
            __syncthreads();
            if (live)
                for (int x0 = 0; x0 < N; x0++) {
                    const T sx = px[x0 + off + dxi] - px[x0 + bx];
                    acc += exp(a * taxi_s(tp[x0], sx, xsign, W) + bl);
                }
        }
        if (live) partial[((size_t)u * N + dti) * N + dxi] = acc;
    }
}

// out = (the unit sums, in unit order) / V; out[0, 0] = 1 (spin.py:129-131, vortex.py:148-150)
__global__ void taxicab_finish(const double *__restrict__ partial, double *out, int N, int nunits) {
    const int64_t V = (int64_t)N * N, i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    double acc = 0.0;
    for (int u = 0; u < nunits; u++) acc += partial[(size_t)u * V + i];
    out[i] = i == 0 ? 1.0 : acc / (double)V;
}

// ---- per-context work buffers ------------------------------------------------------------------------------------
struct CorrCache {
    double2 *A = nullptr, *B = nullptr;  // N x N complex each
    size_t cap = 0;                      // sites
    double2 *tw = nullptr;               // twiddles of N = twN
    int twN = 0;
    char *taxi = nullptr;  // links | Pt | Px | partial | out
    size_t taxi_cap = 0;
    int units_per_group = 1;
    SumWords *sums = nullptr;  // worldline_sums' words, one per workgroup
    size_t sums_cap = 0;
};
std::map<sv_ctx *, CorrCache> g_cache;
std::mutex g_cache_mu;

CorrCache &cache_of(sv_ctx *ctx) {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    return g_cache[ctx];
}

struct NotImplemented : std::runtime_error {
    using std::runtime_error::runtime_error;
};

bool is_pow2(int N) { return N > 0 && (N & (N - 1)) == 0; }

void ensure_fields(CorrCache &c, size_t V) {
    if (V <= c.cap) return;
    (void)hipFree(c.A);
    (void)hipFree(c.B);
    c.A = c.B = nullptr;
    c.cap = 0;
    SV_HIP(hipMalloc((void **)&c.A, V * sizeof(double2)));
    SV_HIP(hipMalloc((void **)&c.B, V * sizeof(double2)));
    c.cap = V;
}

void ensure_twiddles(sv_ctx *ctx, CorrCache &c, int N) {
    if (c.twN == N) return;
    std::vector<double2> h(N / 2);
    for (int k = 0; k < N / 2; k++) {
        const long double ang = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)N;
        h[k] = make_double2((double)cosl(ang), (double)sinl(ang));
    }
    if (N >= 4) h[N / 4] = make_double2(0.0, -1.0);
    (void)hipFree(c.tw);
    c.tw = nullptr;
    c.twN = 0;
    SV_HIP(hipMalloc((void **)&c.tw, (size_t)(N / 2) * sizeof(double2)));
    SV_HIP(hipMemcpyAsync(c.tw, h.data(), h.size() * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    SV_HIP(hipStreamSynchronize(ctx->stream));  // (h goes out of scope)
    c.twN = N;
}

void launch_fft_rows(sv_ctx *ctx, const CorrCache &c, FieldSrc src, double2 *dst, int N, double scale,
                     double scale_im, int planar) {
    int logN = 0;
    while ((1 << logN) < N) logN++;
    const int tpr = std::min(256, N / 2), rows = std::min(256 / tpr, N);
    const size_t lds = (size_t)rows * N * sizeof(double2);
    if (lds > 32768)
        SV_HIP(hipFuncSetAttribute((const void *)fft_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    fft_rows<<<(N + rows - 1) / rows, rows * tpr, lds, ctx->stream>>>(src, dst, c.tw, N, logN, tpr, scale, scale_im,
                                                                      planar),
        SV_LAUNCHED("fft_rows", ctx->stream);
}

void launch_fft_rows(sv_ctx *ctx, const CorrCache &c, FieldSrc src, double2 *dst, int N, double scale) {
    launch_fft_rows(ctx, c, src, dst, N, scale, scale, 0);
}

void launch_transpose(sv_ctx *ctx, const double2 *in, double2 *out, int N) {
    const int tiles = (N + 31) / 32;
    transpose_complex<<<dim3(tiles, tiles), dim3(32, 8), 0, ctx->stream>>>(in, out, N),
        SV_LAUNCHED("transpose_complex", ctx->stream);
}

// The cross-correlation of the field `src` describes (device memory; an F_COMPLEX source may be c.B itself) into
// the host array out (N * N complex128).  path: 0 auto, 1 direct sum, 2 FFT.
// whether a correlation of size N on `path` takes the FFT (else the direct sum); throws where no path serves it
bool takes_fft(int N, int path) {
    if (N < 2) throw std::invalid_argument("correlation: N must be >= 2");
    const int64_t V = (int64_t)N * N;
    const bool fft_ok = is_pow2(N) && N >= FFT_MIN && N <= FFT_MAX, direct_ok = V <= DIRECT_MAX_V;
    if (path < 0 || path > 2) throw std::invalid_argument("correlation: path must be 0 (auto), 1 (direct sum) or 2 (FFT)");
    if (path == 2 && !fft_ok)
        throw NotImplemented("not implemented: the FFT correlation path needs N a power of two with 4 <= N <= 4096, got N = " +
                             std::to_string(N));
    if (path == 1 && !direct_ok)
        throw NotImplemented("not implemented: the direct-sum correlation path needs N * N <= 65536, got N = " +
                             std::to_string(N));
    if (path == 0 && !fft_ok && !direct_ok)
        throw NotImplemented("not implemented: correlation of N = " + std::to_string(N) +
                             " (neither a power of two in 4..4096 nor N * N <= 65536)");
    return path == 2 || (path == 0 && fft_ok);
}

void correlate(sv_ctx *ctx, int N, FieldSrc src, double *out, int path) {
    const bool fft = takes_fft(N, path);
    const int64_t V = (int64_t)N * N;
    CorrCache &c = cache_of(ctx);
    ensure_fields(c, (size_t)V);
    hipEvent_t ev;
    if (fft) {
        ensure_twiddles(ctx, c, N);
        ctx->time_begin(&ev);
        launch_fft_rows(ctx, c, src, c.A, N, 1.0);  // (a row is in LDS before it is written: src may be c.A's twin)
        launch_transpose(ctx, c.A, c.B, N);
        launch_fft_rows(ctx, c, FieldSrc{c.B, F_COMPLEX, 0.0}, c.A, N, 1.0);  // A = F, transposed
        launch_fft_rows(ctx, c, FieldSrc{c.A, F_POWER, 0.0}, c.B, N, 1.0);    // |F|^2 on load
        launch_transpose(ctx, c.B, c.A, N);
        // FFT(|F|^2) = V^2 C: fft(conj fft(f) fft(f)) / sqrt(V) in the ortho convention (compact.py:465-...)
        launch_fft_rows(ctx, c, FieldSrc{c.A, F_COMPLEX, 0.0}, c.B, N, 1.0 / ((double)V * (double)V));
        ctx->time_end(ev, 6);
    } else {
        ctx->time_begin(&ev);
        const double2 *f = (const double2 *)src.p;
        if (src.mode != F_COMPLEX || src.p == c.B) {
            form_field<<<(unsigned)((V + 255) / 256), 256, 0, ctx->stream>>>(src, c.A, V),
                SV_LAUNCHED("form_field", ctx->stream);
            f = c.A;
        }
        const int bs = std::min(256, (N + 63) / 64 * 64);
        correlation_direct<<<dim3(N, (N + bs - 1) / bs), bs, (size_t)3 * N * sizeof(double2), ctx->stream>>>(f, c.B, N),
            SV_LAUNCHED("correlation_direct", ctx->stream);
        ctx->time_end(ev, 2);
    }
    SV_HIP(hipGetLastError());
    SV_HIP(hipMemcpyAsync(out, c.B, (size_t)V * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    SV_HIP(hipStreamSynchronize(ctx->stream));
    ctx->time_collect();
}

// The autocorrelations of the two real fields `src` packs as a + i b, from one transform pass, into the host arrays
// out_aa and out_bb (N * N float64 each; either may be null), C_bb times scale_bb.  path as in correlate.
void correlate_real(sv_ctx *ctx, int N, FieldSrc src, double *out_aa, double *out_bb, int path, double scale_bb) {
    const bool fft = takes_fft(N, path);
    const int64_t V = (int64_t)N * N;
    CorrCache &c = cache_of(ctx);
    ensure_fields(c, (size_t)V);
    hipEvent_t ev;
    if (fft) {
        ensure_twiddles(ctx, c, N);
        ctx->time_begin(&ev);
        launch_fft_rows(ctx, c, src, c.A, N, 1.0);
        launch_transpose(ctx, c.A, c.B, N);
        launch_fft_rows(ctx, c, FieldSrc{c.B, F_COMPLEX, 0.0}, c.A, N, 1.0);  // A = Z, transposed
        FieldSrc pair{c.A, F_POWER_PAIR, 0.0};
        pair.N = N;
        launch_fft_rows(ctx, c, pair, c.B, N, 1.0);  // |A|^2 + i |B|^2 on load: real and even in k, both
        launch_transpose(ctx, c.B, c.A, N);
        // FFT(|A|^2 + i |B|^2) = V^2 (C_aa + i C_bb)
        const double s = 1.0 / ((double)V * (double)V);
        launch_fft_rows(ctx, c, FieldSrc{c.A, F_COMPLEX, 0.0}, c.B, N, s, s * scale_bb, 1);
        ctx->time_end(ev, 6);
    } else {
        ctx->time_begin(&ev);
        form_field<<<(unsigned)((V + 255) / 256), 256, 0, ctx->stream>>>(src, c.A, V),
            SV_LAUNCHED("form_field", ctx->stream);
        const int bs = std::min(256, (N + 63) / 64 * 64);
        correlation_direct_real<<<dim3(N, (N + bs - 1) / bs), bs, (size_t)3 * N * sizeof(double2), ctx->stream>>>(
            c.A, (double *)c.B, N, 1.0, scale_bb),
            SV_LAUNCHED("correlation_direct_real", ctx->stream);
        ctx->time_end(ev, 2);
    }
    SV_HIP(hipGetLastError());
    const double *planes = (const double *)c.B;
    if (out_aa)
        SV_HIP(hipMemcpyAsync(out_aa, planes, (size_t)V * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (out_bb)
        SV_HIP(hipMemcpyAsync(out_bb, planes + V, (size_t)V * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SV_HIP(hipStreamSynchronize(ctx->stream));
    ctx->time_collect();
}

// The sums of a Worldline state (sv_worldline_sums), and whether its fields take the exact integer forms.
bool worldline_exact(const sv_worldline *st, double W_eff) {
    const int64_t Wi = (int64_t)W_eff;
    return !st->v_is_float && (double)Wi == W_eff && Wi >= 1 && Wi < (int64_t(1) << 20);
}

void worldline_sum(sv_worldline *st, double W_eff, sv_worldline_sums *out) {
    sv_ctx *ctx = st->ctx;
    CorrCache &c = cache_of(ctx);
    const int N = st->N;
    const int64_t V = (int64_t)N * N;
    const size_t groups = (size_t)((V + SUM_SITES - 1) / SUM_SITES);
    if (groups > c.sums_cap) {
        (void)hipFree(c.sums);
        c.sums = nullptr;
        c.sums_cap = 0;
        SV_HIP(hipMalloc((void **)&c.sums, groups * sizeof(SumWords)));
        c.sums_cap = groups;
    }
    const bool exact = worldline_exact(st, W_eff);
    const int64_t Wi = exact ? (int64_t)W_eff : 0;
    hipEvent_t ev;
    ctx->time_begin(&ev);
    if (st->v_is_float)
        worldline_sums<double, false><<<(unsigned)groups, SUM_THREADS, 0, ctx->stream>>>(st->m, (const double *)st->v, N,
                                                                                       W_eff, 0, c.sums),
            SV_LAUNCHED("worldline_sums", ctx->stream);
    else if (exact)
        worldline_sums<int64_t, true><<<(unsigned)groups, SUM_THREADS, 0, ctx->stream>>>(st->m, (const int64_t *)st->v, N,
                                                                                       W_eff, Wi, c.sums),
            SV_LAUNCHED("worldline_sums", ctx->stream);
    else
        worldline_sums<int64_t, false><<<(unsigned)groups, SUM_THREADS, 0, ctx->stream>>>(st->m, (const int64_t *)st->v,
                                                                                        N, W_eff, 0, c.sums),
            SV_LAUNCHED("worldline_sums", ctx->stream);
    ctx->time_end(ev, 1);
    SV_HIP(hipGetLastError());
    std::vector<SumWords> h(groups);
    SV_HIP(hipMemcpyAsync(h.data(), c.sums, groups * sizeof(SumWords), hipMemcpyDeviceToHost, ctx->stream));
    SV_HIP(hipStreamSynchronize(ctx->stream));
    ctx->time_collect();
    SumWords t = {0.0, 0.0, 0, 0, 0, 0};
    for (const SumWords &w : h) {
        t.l2 += w.l2;
        t.dl2 += w.dl2;
        t.m0 += w.m0;
        t.m1 += w.m1;
        t.wl2 += w.wl2;
        t.wdl2 += w.wdl2;
    }
    out->links_squared = exact ? (double)t.wl2 / (W_eff * W_eff) : t.l2;
    out->curl_squared = exact ? (double)t.wdl2 / (W_eff * W_eff) : t.dl2;
    out->m0 = t.m0;
    out->m1 = t.m1;
    out->exact = exact ? 1 : 0;
    out->w_links_squared = t.wl2;
    out->w_curl_squared = t.wdl2;
}

// The contact stencil d(delta(unit source on the plaquette at the origin)) (winding.py:189-200) as (site, value)
// entries: delta(s)_0 = s[t, x] - s[t, x - 1], delta(s)_1 = -(s[t, x] - s[t - 1, x]), d(l) = (l_1[t + 1] - l_1) -
// (l_0[x + 1] - l_0), accumulated on the periodic lattice, so coinciding neighbours of a small N add up.
std::map<int64_t, double> contact_stencil(int N) {
    auto at = [N](int t, int x) { return (int64_t)(((t % N) + N) % N) * N + (((x % N) + N) % N); };
    std::map<int64_t, double> l0, l1, out;
    l0[at(0, 0)] += 1.0;
    l0[at(0, 1)] -= 1.0;
    l1[at(0, 0)] -= 1.0;
    l1[at(1, 0)] += 1.0;
    for (const auto &e : l1) {  // entry at site y contributes +1 to d at y - e_t and -1 to d at y
        const int t = (int)(e.first / N), x = (int)(e.first % N);
        out[at(t - 1, x)] += e.second;
        out[at(t, x)] -= e.second;
    }
    for (const auto &e : l0) {
        const int t = (int)(e.first / N), x = (int)(e.first % N);
        out[at(t, x - 1)] -= e.second;
        out[at(t, x)] += e.second;
    }
    return out;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

struct TaxiBuffers {
    void *links, *Pt, *Px;
    double *partial, *out;
    int unit_rows, nunits;
};

TaxiBuffers taxi_buffers(CorrCache &c, int N) {
    if (N < 2 || N > TAXI_MAX_N)
        throw NotImplemented("not implemented: the taxicab correlators need 2 <= N <= " + std::to_string(TAXI_MAX_N) +
                             ", got N = " + std::to_string(N));
    const size_t V = (size_t)N * N;
    TaxiBuffers b;
    b.unit_rows = std::max(1, N / TAXI_UNITS);
    b.nunits = (N + b.unit_rows - 1) / b.unit_rows;
    const size_t o_pt = align256(2 * V * 8), o_px = o_pt + align256((size_t)(2 * N + 1) * N * 8);
    const size_t o_part = o_px + align256((size_t)(2 * N + 1) * N * 8), o_out = o_part + align256(b.nunits * V * 8);
    const size_t total = o_out + align256(V * 8);
    if (total > c.taxi_cap) {
        (void)hipFree(c.taxi);
        c.taxi = nullptr;
        c.taxi_cap = 0;
        SV_HIP(hipMalloc((void **)&c.taxi, total));
        c.taxi_cap = total;
    }
    b.links = c.taxi;
    b.Pt = c.taxi + o_pt;
    b.Px = c.taxi + o_px;
    b.partial = (double *)(c.taxi + o_part);
    b.out = (double *)(c.taxi + o_out);
    return b;
}

// b.links holds the (2, N, N) links (T = double) or W times them (T = int64_t); out: host, N * N float64
template <typename T>
void taxicab(sv_ctx *ctx, CorrCache &c, const TaxiBuffers &b, int N, double a, double bcoef, int dual, double W,
             double *out) {
    const int tcomp = dual ? 1 : 0, xcomp = dual ? 0 : 1, off = dual ? 1 : 0, xsign = dual ? -1 : 1;
    const int64_t V = (int64_t)N * N;
    hipEvent_t ev;
    ctx->time_begin(&ev);
    taxicab_prefix<T><<<(N + 63) / 64, 64, 0, ctx->stream>>>((const T *)b.links, (T *)b.Pt, (T *)b.Px, N, tcomp, xcomp),
        SV_LAUNCHED("taxicab_prefix", ctx->stream);
    const int bs = std::min(256, (N + 63) / 64 * 64);
    const int upg = std::max(1, std::min(c.units_per_group, b.nunits));
    const dim3 grid(N, (N + bs - 1) / bs, (b.nunits + upg - 1) / upg);
    taxicab_sum<T><<<grid, bs, (size_t)(3 * N + 1) * sizeof(T), ctx->stream>>>(
        (const T *)b.Pt, (const T *)b.Px, b.partial, N, off, xsign, a, bcoef, W, b.unit_rows, b.nunits, upg),
        SV_LAUNCHED("taxicab_sum", ctx->stream);
    taxicab_finish<<<(unsigned)((V + 255) / 256), 256, 0, ctx->stream>>>(b.partial, b.out, N, b.nunits),
        SV_LAUNCHED("taxicab_finish", ctx->stream);
    ctx->time_end(ev, 3);
    SV_HIP(hipGetLastError());
    SV_HIP(hipMemcpyAsync(out, b.out, (size_t)V * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SV_HIP(hipStreamSynchronize(ctx->stream));
    ctx->time_collect();
}

template <typename F>
int guarded(sv_ctx *ctx, F &&body) {
    if (!ctx) return -1;
    try {
        SV_HIP(hipSetDevice(ctx->device));
        body();
        return 0;
    } catch (const std::exception &e) {
        ctx->err = e.what();
        return -2;
    }
}

}  // namespace

namespace sv {
void correlators_release(sv_ctx *ctx) {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    auto it = g_cache.find(ctx);
    if (it == g_cache.end()) return;
    (void)hipFree(it->second.A);
    (void)hipFree(it->second.B);
    (void)hipFree(it->second.tw);
    (void)hipFree(it->second.taxi);
    (void)hipFree(it->second.sums);
    g_cache.erase(it);
}
}  // namespace sv

extern "C" {

int sv_ctx_set_taxicab_units(sv_ctx *ctx, int32_t units_per_group) {
    if (!ctx || units_per_group < 0) return -1;
    cache_of(ctx).units_per_group = units_per_group == 0 ? 1 : units_per_group;
    return 0;
}

int sv_villain_spin_spin(sv_villain *st, double *out, int32_t path) {
    if (!st || !out) return -1;
    return guarded(st->ctx, [&] { correlate(st->ctx, st->N, FieldSrc{st->phi[st->cur], F_PHI, 0.0}, out, path); });
}

int sv_worldline_vortex_vortex(sv_worldline *st, double W_eff, double *out, int32_t path) {
    if (!st || !out) return -1;
    return guarded(st->ctx, [&] {
        correlate(st->ctx, st->N, FieldSrc{st->v, st->v_is_float ? F_VFLOAT : F_VINT, 1.0 / W_eff}, out, path);
    });
}

int sv_villain_vortex_vortex(sv_villain *st, double kappa, double *out) {
    if (!st || !out) return -1;
    sv_ctx *ctx = st->ctx;
    return guarded(ctx, [&] {
        CorrCache &c = cache_of(ctx);
        const TaxiBuffers b = taxi_buffers(c, st->N);
        const int64_t V = (int64_t)st->N * st->N;
        villain_links<<<(unsigned)((V + 255) / 256), 256, 0, ctx->stream>>>(st->phi[st->cur], st->n[st->cur],
                                                                            (double *)b.links, st->N),
            SV_LAUNCHED("villain_links", ctx->stream);
        const double pi = TWO_PI / 2.0;
        // exp(-dS), dS = -2 pi kappa (sum(change_n Links) - pi length) (vortex.py:186-187)
        taxicab<double>(ctx, c, b, st->N, 2.0 * pi * kappa, -(2.0 * pi * kappa) * pi, 1, 1.0, out);
    });
}

int sv_worldline_spin_spin(sv_worldline *st, double kappa, double W_eff, double *out) {
    if (!st || !out) return -1;
    sv_ctx *ctx = st->ctx;
    return guarded(ctx, [&] {
        CorrCache &c = cache_of(ctx);
        const TaxiBuffers b = taxi_buffers(c, st->N);
        const int64_t V = (int64_t)st->N * st->N;
        const unsigned grid = (unsigned)((V + 255) / 256);
        // exp(-1 / (2 kappa) (2 Pm + |P|)) (spin.py:222)
        const double a = -1.0 / kappa, bcoef = -1.0 / (2.0 * kappa);
        const int64_t Wi = (int64_t)W_eff;
        if (st->v_is_float) {
            worldline_links<double, false><<<grid, 256, 0, ctx->stream>>>(st->m, (const double *)st->v, b.links, st->N,
                                                                         W_eff, 0),
                SV_LAUNCHED("worldline_links", ctx->stream);
            taxicab<double>(ctx, c, b, st->N, a, bcoef, 0, 1.0, out);
        } else if ((double)Wi == W_eff && Wi >= 1 && Wi < (int64_t(1) << 20)) {
            // integer W: W Links = W m - delta(v) is an integer, the run sums are exact
            worldline_links<int64_t, true><<<grid, 256, 0, ctx->stream>>>(st->m, (const int64_t *)st->v, b.links, st->N,
                                                                         W_eff, Wi),
                SV_LAUNCHED("worldline_links", ctx->stream);
            taxicab<int64_t>(ctx, c, b, st->N, a, bcoef, 0, W_eff, out);
        } else {
            worldline_links<int64_t, false><<<grid, 256, 0, ctx->stream>>>(st->m, (const int64_t *)st->v, b.links, st->N,
                                                                          W_eff, 0),
                SV_LAUNCHED("worldline_links", ctx->stream);
            taxicab<double>(ctx, c, b, st->N, a, bcoef, 0, 1.0, out);
        }
    });
}

int sv_correlation(sv_ctx *ctx, int32_t N, const double *f, double *out, int32_t path) {
    if (!ctx || !f || !out) return -1;
    return guarded(ctx, [&] {
        if (N < 2 || N > FFT_MAX) throw NotImplemented("not implemented: correlation of N = " + std::to_string(N));
        CorrCache &c = cache_of(ctx);
        const size_t V = (size_t)N * N;
        ensure_fields(c, V);
        SV_HIP(hipMemcpyAsync(c.B, f, V * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
        correlate(ctx, N, FieldSrc{c.B, F_COMPLEX, 0.0}, out, path);
    });
}

int sv_villain_action_winding(sv_villain *st, double kappa, double *out_action, double *out_winding, double *scalars,
                              int32_t path) {
    if (!st) return -1;
    sv_ctx *ctx = st->ctx;
    double sums[4];
    const int rc = guarded(ctx, [&] {
        FieldSrc src{st->phi[st->cur], F_VILLAIN_AW, 0.0};
        src.q = st->n[st->cur];
        src.N = st->N;
        src.coef = 0.5 * kappa;
        correlate_real(ctx, st->N, src, out_action, out_winding, path, 1.0);
    });
    if (rc) return rc;
    // S = sum a, exact in fixed point (villain_observables_kernel)
    if (const int rs = sv_villain_observables(st, kappa, sums)) return rs;
    if (out_action) out_action[0] -= sums[0] / ((double)st->N * (double)st->N);  // mean(a) (action.py:99)
    if (scalars)
        for (int i = 0; i < 4; i++) scalars[i] = sums[i];
    return 0;
}

int sv_worldline_observables(sv_worldline *st, double kappa, double W_eff, sv_worldline_sums *out) {
    if (!st || !out) return -1;
    (void)kappa;  // (the sums do not depend on it; the argument keeps the signature of sv_villain_observables)
    return guarded(st->ctx, [&] { worldline_sum(st, W_eff, out); });
}

int sv_worldline_action_winding(sv_worldline *st, double kappa, double W_eff, double *out_action, double *out_winding,
                                sv_worldline_sums *scalars, int32_t path) {
    if (!st) return -1;
    sv_ctx *ctx = st->ctx;
    return guarded(ctx, [&] {
        const int N = st->N;
        const double V = (double)N * (double)N, pi = TWO_PI / 2.0;
        const bool exact = worldline_exact(st, W_eff);
        FieldSrc src{st->m, st->v_is_float ? F_WORLDLINE_AW_VFLOAT : exact ? F_WORLDLINE_AW_EXACT : F_WORLDLINE_AW, 0.0};
        src.q = st->v;
        src.N = N;
        src.coef = 0.5 / kappa;
        src.W = W_eff;
        src.Wi = exact ? (int64_t)W_eff : 0;
        const double norm = (2.0 * pi * kappa) * (2.0 * pi * kappa);
        // (kappa contact - C_bb) / (2 pi kappa)^2 (winding.py:202): the store scales C_bb, the host adds the stencil
        correlate_real(ctx, N, src, out_action, out_winding, path, -1.0 / norm);
        sv_worldline_sums sums;
        worldline_sum(st, W_eff, &sums);
        if (out_action) out_action[0] -= sums.links_squared / 2.0 / kappa / V;  // mean(l^2 / 2 / kappa) (action.py:148-150)
        if (out_winding)
            for (const auto &e : contact_stencil(N)) out_winding[e.first] += kappa * e.second / norm;
        if (scalars) *scalars = sums;
    });
}

int sv_correlation_real(sv_ctx *ctx, int32_t N, const double *a, const double *b, double *out_aa, double *out_bb,
                        int32_t path) {
    if (!ctx || !a) return -1;
    return guarded(ctx, [&] {
        if (N < 2 || N > FFT_MAX) throw NotImplemented("not implemented: correlation of N = " + std::to_string(N));
        takes_fft(N, path);  // (refuses a size before anything is uploaded)
        CorrCache &c = cache_of(ctx);
        const size_t V = (size_t)N * N;
        ensure_fields(c, V);
        double *planes = (double *)c.B;  // the two fields, planar: V double2 hold 2 V doubles
        SV_HIP(hipMemcpyAsync(planes, a, V * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        if (b)
            SV_HIP(hipMemcpyAsync(planes + V, b, V * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        else
            SV_HIP(hipMemsetAsync(planes + V, 0, V * sizeof(double), ctx->stream));
        FieldSrc src{c.B, F_PLANAR, 0.0};
        src.N = N;
        correlate_real(ctx, N, src, out_aa, b ? out_bb : nullptr, path, 1.0);
    });
}

int sv_taxicab_correlator(sv_ctx *ctx, int32_t N, const double *links, double a, double b, int32_t dual, double *out) {
    if (!ctx || !links || !out) return -1;
    return guarded(ctx, [&] {
        CorrCache &c = cache_of(ctx);
        const TaxiBuffers bufs = taxi_buffers(c, N);
        SV_HIP(hipMemcpyAsync(bufs.links, links, (size_t)2 * N * N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        taxicab<double>(ctx, c, bufs, N, a, b, dual != 0, 1.0, out);
    });
}

}  // extern "C"
