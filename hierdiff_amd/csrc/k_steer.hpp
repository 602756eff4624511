// Steered sampling: particle resampling on the restraint energy inside the path loop (hd_set_steer / hd_steer_attach /
// hd_steer_step / hd_steer_read; no reference counterpart).  Included through kernels.hpp.
// The batch is G groups of P rows; group g owns rows g P .. g P + P - 1 (equal masks, contexts and restraint rows: the caller's
// business).  Per transition, behind the network call, guidance and k_restrain_eps:
//   k_steer_weigh      U(b) = (((U_obs + U_pair) + U_anc) + U_fld) + U_tpl of the transition's data prediction x^0 (the fp32 operations of k_restrain_eps,
//                      the energy code of k_restraint_energy), logw[b] += -beta_k (U - U_prev[b]), U_prev[b] = U.  A non-finite U
//                      (or update) is weight 0: logw = -inf.
//   k_steer_resample   per group: m = max logw, w_i = exp(logw_i - m), S = sum w, S2 = sum w^2 in index order (a serial scan by one
//                      thread: the order is a function of P alone), ESS = S^2 / S2.  ESS < rho P: systematic resampling with ONE
//                      uniform u, anc[j] = the smallest i whose inclusive prefix sum exceeds (u + j) / P * S (never past the last
//                      row of positive weight); lineage roots follow, logw = 0.  Otherwise anc[j] = j.  m = -inf (every weight 0):
//                      the group is left alone and counted.
//   k_steer_gather<0>  rows with anc[b] != b: z, eps^ and U_prev of row anc[b] into the topology's scratch
//   k_steer_gather<1>  ... and from the scratch into row b.  Rows with anc[b] == b are not written.  With `hist` (the stochastic
//                      multistep rows, k_post_step<3>) the data prediction x^_{k-1} of the lineage travels the same way.
// u = philox_uniform(seed, id of the group's first row, the transition's draw T - s, ST_UNIFORM_INDEX): words 2 and 3 of the block
// whose words 0 and 1 no normal uses (index / 2 = 2^31 - 1; a molecule has at most 16384 entries), 26 bits each, in double.
// No atomics; every sum has a fixed order.  stats [G][3] = (resampling events, smallest ESS, transitions with every weight 0).
#pragma once
#include "common.hpp"
#include "k_restrain.hpp"
#include "k_restrain_feat.hpp"

#define ST_MAX_P 256
#define ST_UNIFORM_INDEX 0xfffffffeu

// uniform(seed, sample, draw, index) in (0, 1): the counter block of philox_normal, words 2 and 3
HD_DEVINL double philox_uniform(uint64_t seed, uint64_t sample, uint32_t draw, uint32_t index) {
    uint32_t c0 = index >> 1, c1 = draw, c2 = (uint32_t)sample, c3 = (uint32_t)(sample >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const uint64_t v = ((uint64_t)(c2 >> 6) << 26) | (uint64_t)(c3 >> 6);
    return ((double)v + 0.5) * (1.0 / 4503599627370496.0);
}

struct SteerWeighArgs {
    const float* z;         // [B][N][D] z_t
    const float* eps;       // [B][N][D] eps^ (behind guidance and the restraint update)
    const uint8_t* nm;
    RestraintTables t;
    const float* rows;      // device [K][3] {alpha_t, sigma_t, beta_k} (path loop); null: `row`
    float row[3];
    const int* step_ptr;    // device-side path position (graph replay); null: `k`
    int k;
    float nv0;
    double *logw, *uprev;   // [B]
    int B, N, D;
    TemplateTables tp;      // TPL only, behind everything k_steer_weigh<false> reads
    FeatureTables ft;       // FEAT only, behind everything the other instantiations read
};

// Dynamic LDS: N * 3 floats (x^0 of the molecule); FEAT: N * D floats (then its features v [N][F], k_restrain_feat.hpp).
// TPL: templates are attached; U gains U_tpl (rs_template_fit, rs_template_block) behind U_fld.
// FEAT: features are attached; U gains U_feat = U_band + U_sum (ft_energy_block) behind U_tpl.
template <bool TPL, bool FEAT = false>
__global__ __launch_bounds__(256) void k_steer_weigh(SteerWeighArgs a) {
    extern __shared__ float st_x[];
    __shared__ double red[4 * (FEAT ? FT_RED : TPL ? 9 : 3)];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int N = a.N, D = a.D;
    const size_t base = (size_t)b * N * D;
    const float* z = a.z + base;
    const float* eps = a.eps + base;
    const uint8_t* nm = a.nm + (size_t)b * N;
    const int k = a.step_ptr ? *a.step_ptr : a.k;
    const float* row = a.rows ? a.rows + (size_t)k * 3 : a.row;
    const float al = row[0], sg = row[1], beta = row[2];
    const float ra = __fdiv_rn(1.f, al);               // x^0 with the operations and the order of k_restrain_eps
    for (int e = tid; e < 3 * N; e += 256) {
        const int i = e / 3, c = e - 3 * i;
        const size_t o = (size_t)i * D + c;
        st_x[e] = __fmul_rn(__fmul_rn(ra, __fsub_rn(z[o], __fmul_rn(sg, eps[o]))), a.nv0);
    }
    if constexpr (FEAT) ft_data_prediction(z, eps, al, sg, a.ft.nv1, a.ft.nb1, N, D, st_x + 3 * N, tid);
    __syncthreads();
    double U[4];
    rs_energy_block(a.t, b, st_x, nm, N, red, tid, U);
    double utpl = 0.0;
    if constexpr (TPL) {
        __shared__ double tp_fit[HD_MAX_TEMPLATES * RS_FIT];
        rs_template_fit(a.tp, b, st_x, nm, N, red, tp_fit, tid);
        utpl = rs_template_block(a.tp, b, st_x, nm, N, red, tp_fit, tid);
    }
    double ufeat = 0.0;
    if constexpr (FEAT) {
        __shared__ double ft_rowv[FT_ROW];
        double Uf[2];
        ft_energy_block(a.ft, b, st_x + 3 * N, nm, N, D - 3, red, ft_rowv, tid, Uf);
        ufeat = Uf[0] + Uf[1];
    }
    if (tid == 0) {
        const double u3 = (U[0] + U[1]) + U[2];
        const double u4 = a.t.NF ? u3 + U[3] : u3;      // no fields: the old sum's bits
        const double u5 = TPL ? u4 + utpl : u4;
        const double u = FEAT ? u5 + ufeat : u5;
        const double dl = -(double)beta * (u - a.uprev[b]);
        // (finite: |v| < inf, false for a NaN.  Not v - v == 0: with v a product the compiler contracts that into the product's rounding error)
        a.logw[b] = (fabs(u) < HUGE_VAL && fabs(dl) < HUGE_VAL) ? a.logw[b] + dl : -HUGE_VAL;
        a.uprev[b] = u;
    }
}

struct SteerState {
    double *logw, *uprev;   // [B]
    int *root, *anc;        // [B] index within the group of the initial particle; source row of this transition's gather
    double* stats;          // [G][3]
};

struct SteerResampleArgs {
    SteerState st;
    double ess;             // rho
    uint64_t seed, base;
    uint32_t draw;
    const uint32_t* draw_ptr;               // device words (graph replay); override draw / base
    const unsigned long long* base_ptr;
    int P;
};

// One workgroup per group.
__global__ __launch_bounds__(256) void k_steer_resample(SteerResampleArgs a) {
    __shared__ double w[ST_MAX_P], cum[ST_MAX_P];
    __shared__ int rt[ST_MAX_P];
    __shared__ double sc[3];                            // max, S, whether to resample
    __shared__ int last_s;
    const int tid = threadIdx.x, g = blockIdx.x, P = a.P;
    const size_t r0 = (size_t)g * P;
    if (tid < P) { w[tid] = a.st.logw[r0 + tid]; rt[tid] = a.st.root[r0 + tid]; }
    __syncthreads();
    if (tid == 0) {
        double m = -HUGE_VAL;
        for (int i = 0; i < P; ++i) m = w[i] > m ? w[i] : m;
        sc[0] = m;
    }
    __syncthreads();
    const double m = sc[0];
    double* stats = a.st.stats + (size_t)g * 3;
    if (!(m > -HUGE_VAL)) {                             // every weight is 0: uniform over the workgroup
        if (tid < P) a.st.anc[r0 + tid] = (int)r0 + tid;
        if (tid == 0) stats[2] += 1.0;
        return;
    }
    if (tid < P) w[tid] = exp(w[tid] - m);
    __syncthreads();
    if (tid == 0) {
        double s = 0.0, s2 = 0.0;
        int last = 0;
        for (int i = 0; i < P; ++i) {
            s += w[i]; s2 += w[i] * w[i]; cum[i] = s;
            if (w[i] > 0.0) last = i;
        }
        const double ess = s * s / s2;
        if (ess < stats[1]) stats[1] = ess;
        const bool go = ess < a.ess * (double)P;
        if (go) stats[0] += 1.0;
        sc[1] = s; sc[2] = go ? 1.0 : 0.0;
        last_s = last;
    }
    __syncthreads();
    if (tid >= P) return;
    if (sc[2] == 0.0) { a.st.anc[r0 + tid] = (int)r0 + tid; return; }
    const uint64_t base = a.base_ptr ? (uint64_t)*a.base_ptr : a.base;
    const uint32_t draw = a.draw_ptr ? *a.draw_ptr : a.draw;
    const double u = philox_uniform(a.seed, base + (uint64_t)r0, draw, ST_UNIFORM_INDEX);
    const double target = (u + (double)tid) / (double)P * sc[1];
    int lo = 0, hi = P;                                 // the smallest i with cum[i] > target
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > target) hi = mid; else lo = mid + 1;
    }
    const int src = lo < last_s ? lo : last_s;
    a.st.anc[r0 + tid] = (int)r0 + src;
    a.st.root[r0 + tid] = rt[src];
    a.st.logw[r0 + tid] = 0.0;
}

struct SteerGatherArgs {
    float *z, *eps;         // [B][N][D]
    float* scratch;         // [3][B][N][D]
    float* hist;            // [B][N][D] x^_{k-1} of the stochastic multistep rows, or null
    double *uprev, *us;     // [B], and its scratch
    const int* anc;
    int B, total;           // total = N * D
};

template <int BACK>
__global__ __launch_bounds__(256) void k_steer_gather(SteerGatherArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int src = a.anc[b];
    if (src == b) return;                               // uniform over the workgroup
    const size_t all = (size_t)a.B * a.total, ob = (size_t)b * a.total;
    if constexpr (BACK == 0) {
        const size_t os = (size_t)src * a.total;
        for (int e = tid; e < a.total; e += 256) { a.scratch[ob + e] = a.z[os + e]; a.scratch[all + ob + e] = a.eps[os + e]; }
        if (a.hist) for (int e = tid; e < a.total; e += 256) a.scratch[2 * all + ob + e] = a.hist[os + e];
        if (tid == 0) a.us[b] = a.uprev[src];
    } else {
        for (int e = tid; e < a.total; e += 256) { a.z[ob + e] = a.scratch[ob + e]; a.eps[ob + e] = a.scratch[all + ob + e]; }
        if (a.hist) for (int e = tid; e < a.total; e += 256) a.hist[ob + e] = a.scratch[2 * all + ob + e];
        if (tid == 0) a.uprev[b] = a.us[b];
    }
}

// the state of a chain's start: logw = U_prev = 0, every row its own root, no events, smallest ESS = P
__global__ void k_steer_init(SteerState st, int B, int P) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    st.logw[b] = 0.0; st.uprev[b] = 0.0; st.root[b] = b % P; st.anc[b] = b;
    if (b % P == 0) { double* s = st.stats + (size_t)(b / P) * 3; s[0] = 0.0; s[1] = (double)P; s[2] = 0.0; }
}
