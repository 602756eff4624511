// Feature restraints: bands and molecule-wide sums on the features h of the data prediction (hd_restraint_features / hd_restrain_feat
// / hd_restraint_feature_energy; no reference counterpart).  Included through kernels.hpp.
//   k_restrain_feat             eps_h += clip(s_b lambda_k ratio dU_feat/dv) with U_feat evaluated on the transition's data prediction
//   k_restraint_feature_energy  (U_band, U_sum) and the m_r per molecule, in double, for given data-unit features
// v, in data units, for a valid node i and channel c in [0, F), F = D - 3, with the operations and the order of k_chain_frame<1> (the
// bits record="x0" shows):  v_ic = fadd(fmul(fmul(1 / alpha_t, fsub(z, fmul(sigma_t, eps^))), nv1), nb1)
// BANDS  lo, hi, k [band_rows][W][F], W <= N (nodes i >= W have none).  Element (i, c) is active when node i is valid, k_ic > 0 and v_ic
//        is finite:  U_band = 1/2 sum k (max(0, v - hi)^2 + max(0, lo - v)^2),  dU/dv = k (max(0, v - hi) - max(0, lo - v))
// SUMS   at most HD_MAX_FEATURE_SUMS rows r: coef [sum_rows][S][F], f [sum_rows][S][4] = (lo, hi, k, reduce: 0 sum, 1 mean)
//        s_r = sum_{i valid} sum_c coef_rc v_ic,  n = valid nodes,  m_r = s_r or s_r / n,
//        U_sum = 1/2 sum_r k_r (max(0, m_r - hi_r)^2 + max(0, lo_r - m_r)^2),  dU/dv_ic += k_r (...) coef_rc (1 or 1 / n)
//        A row is inactive when k_r <= 0 or n = 0, and contributes nothing when a valid v it reads with a non-zero coefficient is
//        not finite.
// rows = 1 (shared) or B.  One workgroup (256 threads) per molecule as k_restrain_eps.  Every thread sums its strided share of the N * F
// elements in double - U_band, the S row sums, how many non-finite values each row read, n - then ONE guide_block_sum over the
// FT_RED values, so every order depends on (N, F, S) alone.  Thread 0 leaves the m_r and the factors k_r (...) (1 or 1 / n) in LDS.
// The step of node i is then gathered by one aligned group of FT_GROUP lanes (lane l: the channels l, l + FT_GROUP, ...): per
// channel the sum terms in row order - formed once per channel, they are the same for every node - then the band; the clip on the
// Euclidean norm over the node's F steps (per-lane partial sums, then an xor butterfly inside the group; apart from the position
// step's clip); no mean is removed (features have no centre-of-gravity constraint).
// An element whose step is exactly 0 keeps its bits; position columns and masked rows are never written.  No atomics, nothing goes to
// global memory between the reduction and the write.  Draws nothing.  It does not read the fixed mask: features have no frame.
#pragma once
#include "common.hpp"
#include "k_guide.hpp"

#ifndef HD_MAX_FEATURE_SUMS
#define HD_MAX_FEATURE_SUMS 8
#endif
#define FT_RED (2 * HD_MAX_FEATURE_SUMS + 2)   // doubles per thread: s_r [8], non-finite reads of row r [8], U_band, n
#define FT_ROW (2 * HD_MAX_FEATURE_SUMS)       // doubles of LDS behind the reduction: m_r [8], the factor of row r [8]
#define FT_GROUP 8                             // lanes that share one node's step

struct FeatureTables {
    const float *lo, *hi, *k;   // [band_rows][W][F]
    const float* coef;          // [sum_rows][S][F]
    const float* sum_f;         // [sum_rows][S][4] = (lo, hi, k, reduce)
    int band_rows, W, sum_rows, S;      // W == 0: no bands; S == 0: no sums (nothing of that family is read)
    float nv1, nb1;
};

struct RestrainFeatArgs {
    const float* z;         // [B][N][D] z_t
    const float* eps;       // [B][N][D] network output, behind guidance and k_restrain_eps
    float* out;             // [B][N][D]; may be eps itself (then only the feature columns of valid nodes are written)
    const uint8_t* nm;      // [B*N] node mask bytes
    FeatureTables t;
    const float* scale;     // [scale_rows] s_b
    const float* rows;      // device [K][4] {alpha_t, sigma_t, lambda_k, clip_k} (path loop); null: `row`
    float row[4];
    const int* step_ptr;    // device-side path position (graph replay); null: `k`
    int k;
    float ratio;            // lambda^h_k = lambda_k ratio
    int scale_rows, B, N, D;
};

struct FeatureEnergyArgs {
    const float* h;         // [B][N][F] features in data units
    const uint8_t* nm;
    FeatureTables t;
    double* out;            // [B][2] (U_band, U_sum)
    double* sums;           // [B][S] m_r (0 for a row that is inactive or contributes nothing); null: not wanted
    int B, N, F;
};

HD_DEVINL bool ft_finite(float v) { return fabsf(v) < HUGE_VALF; }

// v outside [lo, hi]: the signed distance to the nearer bound (dU/dv = k d, U = 1/2 k d^2); inside or on a bound: 0.
HD_DEVINL double ft_excess(double v, double lo, double hi) {
    if (v > hi) return v - hi;
    if (v < lo) return v - lo;
    return 0.0;
}

// dU_band/dv of element (i, c) of molecule b at the value v (0 when the element is inactive; the caller knows the node valid).
HD_DEVINL double ft_band_grad(const FeatureTables& t, int b, int F, int i, int c, float v) {
    if (i >= t.W || !ft_finite(v)) return 0.0;
    const size_t o = ((size_t)(t.band_rows == 1 ? 0 : b) * t.W + i) * F + c;
    const float k = t.k[o];
    if (!(k > 0.f)) return 0.0;
    return (double)k * ft_excess((double)v, (double)t.lo[o], (double)t.hi[o]);
}

// (U_band, U_sum) of the molecule b at the features v [N][F] (data units; global memory or LDS) into U, in every thread; thread 0 leaves
// m_r in rowv[r] and the factor k_r (max(0, m - hi) - max(0, lo - m)) (1 or 1 / n) in rowv[HD_MAX_FEATURE_SUMS + r], visible to every
// thread on return.  `red`: 4 * FT_RED doubles of LDS.  The one energy code of k_restrain_feat, k_restraint_feature_energy and
// k_steer_weigh<*, true>.  Every index into the per-thread arrays is a constant after unrolling: they live in registers.
HD_DEVINL void ft_energy_block(const FeatureTables& t, int b, const float* v, const uint8_t* nm, int N, int F, double* red, double* rowv,
                               int tid, double (&U)[2]) {
    double s[FT_RED];
#pragma unroll
    for (int j = 0; j < FT_RED; ++j) s[j] = 0.0;
    const float* coef = t.coef + (size_t)(t.sum_rows == 1 ? 0 : b) * t.S * F;
    const size_t brow = (size_t)(t.band_rows == 1 ? 0 : b) * t.W * F;
    for (int e = tid; e < N * F; e += 256) {
        const int i = e / F, c = e - i * F;
        if (!nm[i]) continue;
        if (c == 0) s[FT_RED - 1] += 1.0;
        const float ve = v[e];
        const bool fin = ft_finite(ve);
#pragma unroll
        for (int r = 0; r < HD_MAX_FEATURE_SUMS; ++r) {
            if (r < t.S) {
                const float cf = coef[(size_t)r * F + c];
                if (cf != 0.f) {
                    if (fin) s[r] += (double)cf * (double)ve;
                    else s[HD_MAX_FEATURE_SUMS + r] += 1.0;
                }
            }
        }
        if (fin && i < t.W) {
            const size_t o = brow + (size_t)i * F + c;
            const float k = t.k[o];
            if (k > 0.f) {
                const double d = ft_excess((double)ve, (double)t.lo[o], (double)t.hi[o]);
                s[FT_RED - 2] += 0.5 * (double)k * d * d;
            }
        }
    }
    guide_block_sum<FT_RED>(s, red, tid);
    const double n = s[FT_RED - 1];
    const float* sf = t.sum_f + (size_t)(t.sum_rows == 1 ? 0 : b) * t.S * 4;
    double us = 0.0;
#pragma unroll
    for (int r = 0; r < HD_MAX_FEATURE_SUMS; ++r) {
        double m = 0.0, fac = 0.0;
        if (r < t.S) {
            const float k = sf[4 * r + 2];
            if (k > 0.f && n > 0.0 && s[HD_MAX_FEATURE_SUMS + r] == 0.0) {
                const bool mean = sf[4 * r + 3] != 0.f;
                m = mean ? s[r] / n : s[r];
                const double d = ft_excess(m, (double)sf[4 * r], (double)sf[4 * r + 1]);
                us += 0.5 * (double)k * d * d;
                fac = mean ? (double)k * d / n : (double)k * d;
            }
        }
        if (tid == 0) { rowv[r] = m; rowv[HD_MAX_FEATURE_SUMS + r] = fac; }
    }
    __syncthreads();
    U[0] = s[FT_RED - 2];
    U[1] = us;
}

// The data prediction's features of the molecule into v [N][F] (LDS), with the operations and the order of k_chain_frame<1>.  The
// caller's barrier makes them visible.
HD_DEVINL void ft_data_prediction(const float* z, const float* eps, float al, float sg, float nv1, float nb1, int N, int D, float* v,
                                  int tid) {
    const int F = D - 3;
    const float ra = __fdiv_rn(1.f, al);
    for (int e = tid; e < N * F; e += 256) {
        const int i = e / F, c = e - i * F;
        const size_t o = (size_t)i * D + 3 + c;
        v[e] = __fadd_rn(__fmul_rn(__fmul_rn(ra, __fsub_rn(z[o], __fmul_rn(sg, eps[o]))), nv1), nb1);
    }
}

// The sum terms of dU_feat/dv of channel c, in row order (the same for every valid node of the molecule).
HD_DEVINL double ft_sum_grad(const float* coef, const double* fac, int S, int F, int c) {
    double g = 0.0;
    for (int r = 0; r < S; ++r) g += fac[r] * (double)coef[(size_t)r * F + c];
    return g;
}

// Dynamic LDS: N * F floats (v of the molecule).
__global__ __launch_bounds__(256) void k_restrain_feat(RestrainFeatArgs a) {
    extern __shared__ float ft_v[];
    __shared__ double red[4 * FT_RED];
    __shared__ double rowv[FT_ROW];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = a.N, D = a.D, F = D - 3, total = N * D;
    const size_t base = (size_t)b * total;
    const float* z = a.z + base;
    const float* eps = a.eps + base;
    float* out = a.out + base;
    const uint8_t* nm = a.nm + (size_t)b * N;
    if (out != eps)
        for (int e = tid; e < total; e += 256) out[e] = eps[e];
    const int k = a.step_ptr ? *a.step_ptr : a.k;
    const float* row = a.rows ? a.rows + (size_t)k * 4 : a.row;
    const float al = row[0], sg = row[1], lam = row[2], clip = row[3];
    const double sl = (double)a.scale[a.scale_rows == 1 ? 0 : b] * ((double)lam * (double)a.ratio);
    if (sl == 0.0) return;                             // uniform over the workgroup: nothing (more) is written
    ft_data_prediction(z, eps, al, sg, a.t.nv1, a.t.nb1, N, D, ft_v, tid);
    __syncthreads();
    double U[2];
    ft_energy_block(a.t, b, ft_v, nm, N, F, red, rowv, tid, U);
    const double* fac = rowv + HD_MAX_FEATURE_SUMS;
    const float* coef = a.t.coef + (size_t)(a.t.sum_rows == 1 ? 0 : b) * a.t.S * F;
    // The sum terms are the same for every node: one thread per channel forms them once, into `red` (the barrier at the end of
    // ft_energy_block lies behind its last read).  More channels than `red` holds: every lane forms its own, the same bits.
    double* gs = red;
    const bool staged = F <= 4 * FT_RED;               // uniform over the grid
    if (staged) {
        for (int c = tid; c < F; c += 256) gs[c] = ft_sum_grad(coef, fac, a.t.S, F, c);
        __syncthreads();
    }
    // The step of node i is gathered by ONE aligned group of FT_GROUP lanes, lane l taking the channels l, l + FT_GROUP, ...: node i
    // belongs to group (i mod 256 / FT_GROUP) whatever B is, so the order of the norm's sum depends on F alone.
    const bool clips = clip - clip == 0.f;             // finite; uniform over the grid
    const int l = tid & (FT_GROUP - 1), grp = tid / FT_GROUP;
    for (int i0 = 0; i0 < N; i0 += 256 / FT_GROUP) {   // uniform trip count: the shuffles below see whole groups
        const int i = i0 + grp;
        const bool on = i < N && nm[i];
        double f = 1.0;
        if (clips) {
            double q = 0.0;
            if (on)
                for (int c = l; c < F; c += FT_GROUP) {
                    const double d = sl * ((staged ? gs[c] : ft_sum_grad(coef, fac, a.t.S, F, c)) + ft_band_grad(a.t, b, F, i, c, ft_v[i * F + c]));
                    q += d * d;
                }
#pragma unroll
            for (int o = FT_GROUP / 2; o > 0; o >>= 1) q += __shfl_xor(q, o);
            const double len = sqrt(q);
            if (len > (double)clip) f = (double)clip / len;
        }
        if (!on) continue;
        for (int c = l; c < F; c += FT_GROUP) {
            double d = sl * ((staged ? gs[c] : ft_sum_grad(coef, fac, a.t.S, F, c)) + ft_band_grad(a.t, b, F, i, c, ft_v[i * F + c]));
            if (f != 1.0) d *= f;
            if (d == 0.0) continue;                    // an unmoved entry keeps its bits (-0 included)
            const size_t o = (size_t)i * D + 3 + c;
            out[o] = (float)((double)eps[o] + d);
        }
    }
}

__global__ __launch_bounds__(256) void k_restraint_feature_energy(FeatureEnergyArgs a) {
    __shared__ double red[4 * FT_RED];
    __shared__ double rowv[FT_ROW];
    const int tid = threadIdx.x, b = blockIdx.x;
    double U[2];
    ft_energy_block(a.t, b, a.h + (size_t)b * a.N * a.F, a.nm + (size_t)b * a.N, a.N, a.F, red, rowv, tid, U);
    if (tid < 2) a.out[(size_t)b * 2 + tid] = tid == 0 ? U[0] : U[1];
    if (a.sums && tid < a.t.S) a.sums[(size_t)b * a.t.S + tid] = rowv[tid];
}
